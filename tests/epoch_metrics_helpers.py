"""Shared by the epoch-metrics and EnsembleTrainer tests: the golden of ``tests/golden/make_epoch_metrics_golden.py``
(the reference's ``EnsembleTrainer`` on canned logits), integer counts restated in numpy, and the comparison of a
metric dict with a recorded one."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THRESHOLDS = np.linspace(0.05, 0.95, 19, dtype=np.float32)
CE_WEIGHT = [0.7, 1.3]  # the criterion of the recorded per-case losses
# floating metrics are ratios of the same integers on both sides: 1e-12 leaves room for another, equivalent order of
# operations and nothing more (the formulas agree with sklearn 1.7.2 to 1.1e-16 over random cases with ties)
FLOAT_TOL = 1e-12
INT_KEYS = ("confusion_matrix",)
EXACT_KEYS = ("best_thr_accuracy", "best_thr_f1")

_cache = {}


def load():
    """(arrays, results) of the golden, read once"""
    if not _cache:
        _cache["a"] = dict(np.load(os.path.join(GOLDEN, "epoch_metrics.npz")))
        with open(os.path.join(GOLDEN, "epoch_metrics.json")) as f:
            _cache["r"] = json.load(f)
    return _cache["a"], _cache["r"]


def case_names():
    return list(load()[1]["cases"])


def numpy_counts(probs, labels, preds, thresholds=THRESHOLDS):
    """the integers of ``dfd_metrics_finalize`` from fp32 probabilities, labels (anything but 0 / 1: skipped) and
    argmax predictions; every comparison in fp32"""
    probs = np.asarray(probs, dtype=np.float32)
    labels, preds = np.asarray(labels), np.asarray(preds)
    pos, neg = labels == 1, labels == 0
    pp, pn = probs[pos], np.sort(probs[neg])
    less = np.searchsorted(pn, pp, side="left")
    equal = np.searchsorted(pn, pp, side="right") - less
    thr = np.asarray(thresholds, dtype=np.float32)
    return {
        "n_pos": int(pos.sum()), "n_neg": int(neg.sum()),
        "tn": int((neg & (preds == 0)).sum()), "fp": int((neg & (preds == 1)).sum()),
        "fn": int((pos & (preds == 0)).sum()), "tp": int((pos & (preds == 1)).sum()),
        "u2": int(2 * less.sum() + equal.sum()),
        "thresholds": [float(t) for t in thr],
        "tp_t": [int((pp >= t).sum()) for t in thr], "fp_t": [int((pn >= t).sum()) for t in thr],
    }


def assert_metrics(got, ref, keys=None, loss_rel=None, what=""):
    """``got`` against a recorded dict: the same keys (or ``keys`` of them), integers and chosen thresholds exactly,
    floats within FLOAT_TOL; ``loss`` exactly, or within ``loss_rel`` relative where another kernel computed it"""
    if keys is None:
        assert set(got) == set(ref), (what, sorted(got), sorted(ref))
        keys = list(ref)
    for k in keys:
        g, r = got[k], ref[k]
        if k in INT_KEYS or k in EXACT_KEYS:
            assert g == r, (what, k, g, r)
        elif k == "loss":
            if loss_rel is None:
                assert g == r, (what, k, g, r)
            else:
                assert abs(g - r) <= loss_rel * abs(r), (what, k, g, r)
        else:
            assert isinstance(g, float) and abs(g - r) <= FLOAT_TOL, (what, k, g, r)


def sequential_mean(losses):
    """``total_loss += loss.item()`` over the batches, ``/ len(loader)``"""
    tot = 0.0
    for v in losses:
        tot += float(v)
    return tot / len(losses)
