"""Epoch metrics without a GPU.

* ``metrics.metrics_from_counts`` against ``tests/golden/epoch_metrics.json``: the reference's
  ``EnsembleTrainer.validate`` / ``train_epoch`` (sklearn underneath) on canned logits.  The counts come from numpy
  on the golden's inputs (the recorded fp32 probabilities of torch's CPU softmax); integers, chosen thresholds,
  confusion matrices and absent keys match exactly, floating metrics within 1e-12 (``epoch_metrics_helpers``), the
  loss -- the same sequential fp64 sum of the recorded step losses -- exactly.
* the support-weighted precision / recall / F1 against sklearn's recorded ones.
* the C ABI: both launchers return -1 on bad arguments, before any device call.
* operator registration, fake shapes, argument checks of ``EpochMetrics`` that need no device.
"""
import ctypes

import numpy as np
import pytest
import torch

import epoch_metrics_helpers as eh
from deepfake_amd import _lib, metrics, ops


def _dict_for(name, average="binary"):
    A, R = eh.load()
    z, y = A[f"{name}/logits"], A[f"{name}/labels"]
    c = eh.numpy_counts(A[f"{name}/probs"], y, (z[:, 1] > z[:, 0]).astype(np.int64))
    return metrics.metrics_from_counts(c["n_pos"], c["n_neg"], c["tn"], c["fp"], c["fn"], c["tp"], c["u2"],
                                       c["thresholds"], c["tp_t"], c["fp_t"],
                                       loss=eh.sequential_mean(A[f"{name}/losses"]), average=average)


@pytest.mark.parametrize("name", eh.case_names())
def test_metrics_from_counts_matches_reference(name):
    ref = eh.load()[1]["cases"][name]
    got = _dict_for(name)
    eh.assert_metrics(got, ref["validate"], what=name)
    if "train_epoch" in ref:
        eh.assert_metrics(got, ref["train_epoch"], keys=list(ref["train_epoch"]), what=name)
    w = _dict_for(name, average="weighted")
    eh.assert_metrics(w, ref["weighted"], keys=list(ref["weighted"]), what=name)
    for k in ("accuracy", "auc", "confusion_matrix"):
        assert w[k] == got[k]


def test_golden_covers_the_corner_cases():
    A, R = eh.load()
    assert R["thresholds"] == [float(t) for t in eh.THRESHOLDS]
    cases = R["cases"]
    assert {f"n{n}" for n in (1, 2, 63, 64, 65, 257, 513, 1031)} <= set(cases)
    assert cases["all_real"]["validate"]["confusion_matrix"] == [[40]]
    for name in ("n1", "all_real", "all_fake"):  # one class: auc 0.5 and no sweep
        assert cases[name]["validate"]["auc"] == 0.5 and "best_thr_accuracy" not in cases[name]["validate"]
    assert cases["all_wrong"]["validate"]["accuracy"] == 0.0
    assert (A["unlabelled/labels"] == -1).sum() == 30
    z = A["argmax_tie/logits"]
    assert (z[:, 0] == z[:, 1]).sum() >= 3
    assert {1, 3, 32} <= set(A["mixed_batches/batches"].tolist())
    for name in cases:  # exact ties are present in number
        z = A[f"{name}/logits"]
        assert len(z) <= 2 or len(z) - len(np.unique(z, axis=0)) >= len(z) // 4
    run = R["run"]
    assert [p["select_metric"] for p in run["plan"]] == ["f1_thr", "acc", "no_such_metric"]
    assert [a["best_metrics"]["select_metric"] for a in run["after"]] == ["f1_thr", "acc", "accuracy"]
    assert "checkpoint_epoch_10.pt" in run["after"][1]["files"]


def test_first_strictly_greater_threshold_wins():
    # two thresholds with the same accuracy: the first is kept
    m = metrics.metrics_from_counts(2, 2, 1, 1, 1, 1, 4, [0.25, 0.5, 0.75], [2, 2, 1], [1, 1, 0])
    assert m["best_thr_accuracy"] == 0.25 and m["accuracy_thr"] == 0.75
    assert m["best_thr_f1"] == 0.25 and m["f1_thr"] == 0.8
    assert m["auc"] == 0.5


def test_from_counts_corner_cases():
    m = metrics.metrics_from_counts(0, 5, 5, 0, 0, 0, 0, [0.5], [0], [0])
    assert m["confusion_matrix"] == [[5]] and m["auc"] == 0.5 and m["accuracy"] == 1.0
    assert (m["precision"], m["recall"], m["f1"]) == (0.0, 0.0, 0.0) and "f1_thr" not in m
    m = metrics.metrics_from_counts(0, 5, 3, 2, 0, 0, 0)
    assert m["confusion_matrix"] == [[3, 2], [0, 0]]
    m = metrics.metrics_from_counts(0, 0, 0, 0, 0, 0, 0)
    assert m["confusion_matrix"] == [] and m["accuracy"] == 0.0 and m["auc"] == 0.5
    with pytest.raises(ValueError):
        metrics.metrics_from_counts(1, 1, 1, 0, 0, 1, 2, average="macro")
    with pytest.raises(ValueError):
        metrics.metrics_from_counts(3, 1, 1, 0, 0, 1, 2)


def test_launchers_refuse_bad_arguments():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)  # never dereferenced: the launchers refuse before any launch
    p = ctypes.addressof(buf)
    thr = (ctypes.c_float * 33)(*([0.5] * 33))
    for B in (0, -3):
        assert lib.dfd_metrics_append(None, p, p, p, B, 0, 64, p, p, p) == -1
        assert b"B >= 1" in lib.dfd_last_error()
    assert lib.dfd_metrics_append(None, p, p, p, 4, -1, 64, p, p, p) == -1
    assert lib.dfd_metrics_append(None, p, p, p, 4, 61, 64, p, p, p) == -1  # rows past the buffers' capacity
    for k in (1, 2, 7, 8, 9):  # logits, labels, probs, tags, loss sums; the loss (3) may be null
        args = [None, p, p, p, 4, 0, 64, p, p, p]
        args[k] = None
        assert lib.dfd_metrics_append(*args) == -1
        assert b"null" in lib.dfd_last_error()
    assert lib.dfd_metrics_finalize(None, p, p, -1, thr, 19, p) == -1
    assert lib.dfd_metrics_finalize(None, p, p, 8, thr, 33, p) == -1
    assert b"32 thresholds" in lib.dfd_last_error()
    for k in (1, 2, 4, 6):  # probs, tags, thresholds, result
        args = [None, p, p, 8, thr, 19, p]
        args[k] = None
        assert lib.dfd_metrics_finalize(*args) == -1
        assert b"null" in lib.dfd_last_error()


def test_ops_registered_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert not set(ops.METRICS_OPS) & (set(ops.OPS) | set(ops.LOSS_OPS) | set(ops.AUGMENT_OPS))
    for name in ops.METRICS_OPS:
        assert getattr(torch.ops.dfd, name).default._schema.name == f"dfd::{name}"
    schema = str(torch.ops.dfd.metrics_append.default._schema)
    for state in ("probs", "tags", "loss_sums"):  # the op mutates its state tensors
        assert f"!) {state}" in schema, schema
    with FakeTensorMode():
        probs, tags = torch.empty(16), torch.empty(16, dtype=torch.uint8)
        out = torch.ops.dfd.metrics_finalize(probs, tags, 9, [0.5])
        assert out.shape == (ops.METRICS_RESULT_WORDS,) and out.dtype == torch.int64
        assert torch.ops.dfd.metrics_append(torch.empty(3, 2), torch.empty(3, dtype=torch.long), None, 0, probs, tags,
                                            torch.empty(2, dtype=torch.float64)) is None


def test_cpu_refused():
    with pytest.raises(RuntimeError):
        metrics.EpochMetrics("cpu")
    with pytest.raises(NotImplementedError):
        torch.ops.dfd.metrics_finalize(torch.zeros(4), torch.zeros(4, dtype=torch.uint8), 4, [0.5])


def test_ensemble_trainer_has_the_reference_interface():
    import inspect

    from deepfake_amd.trainer import EnsembleTrainer

    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(EnsembleTrainer.__init__) == ["self", "model", "device", "checkpoint_dir", "ensemble_method"]
    assert sig(EnsembleTrainer.train_epoch) == ["self", "train_loader", "optimizer", "criterion", "epoch"]
    assert sig(EnsembleTrainer.validate) == ["self", "val_loader", "criterion", "epoch"]
    assert sig(EnsembleTrainer.train) == ["self", "train_loader", "val_loader", "epochs", "lr", "weight_decay",
                                          "start_epoch", "class_weights", "select_metric"]
    d = inspect.signature(EnsembleTrainer.__init__).parameters
    assert (d["device"].default, d["checkpoint_dir"].default, d["ensemble_method"].default) == (
        "cuda", "checkpoints/ensemble", "weighted")
    for name in ("prepare_optimizers", "_infer_class_weights", "_save_checkpoint", "_save_calibration", "_save_history"):
        assert callable(getattr(EnsembleTrainer, name))
