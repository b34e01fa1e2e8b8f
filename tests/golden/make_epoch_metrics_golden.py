"""Golden fixture for the device-side epoch metrics and the ``EnsembleTrainer`` epoch loop:
``epoch_metrics.npz`` (inputs) and ``epoch_metrics.json`` (recorded results).

Drives the REFERENCE ``EnsembleTrainer`` (``src/ensemble_trainer.py``, imported from a checkout of the reference;
development machine only, needs sklearn) on the CPU with a stub model that returns canned logits ``+ 0 * w``:

* ``validate`` over the cases of ``CASES`` (and ``train_epoch`` over one of them): the metric dicts, the step
  losses it saw and the fake-class probabilities of torch's CPU softmax;
* three ``train(...)`` calls on one trainer, 12 epochs in all: ``select_metric='f1_thr'`` with inferred class
  weights (epochs 1-5), the alias ``'acc'`` (6-11, crosses the every-10th save) and an unknown name (12); the
  ``training_history.csv`` text, ``calibration_best.json``, ``best_metrics`` and the checkpoint files after each.

The device's ``expf`` need not round the way torch's CPU softmax does, so the inputs are built, and ASSERTED, to keep
the reference's metrics independent of the last bit of a probability: two rows have bit-identical logits (exact
ties, about a third of the rows) or fake-probabilities at least 1e-5 apart; every probability is at least 1e-4 from
all 19 sweep thresholds; ``|z1 - z0| <= 8``; and ``z1 != z0`` except in the argmax-tie case, whose tied rows have
the probability 0.5 exactly on any softmax (1 / (1 + 1)) and are exempt from the threshold rule.

    python tests/golden/make_epoch_metrics_golden.py /path/to/reference
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

THRESHOLDS = np.linspace(0.05, 0.95, 19, dtype=np.float32)
# the probabilities the distinct rows take: an even grid, without the points near a sweep threshold
GRID = np.linspace(0.002, 0.998, 1200)
GRID = GRID[np.abs(GRID[:, None] - THRESHOLDS[None, :].astype(np.float64)).min(axis=1) > 3e-4]

# name: (rows, fraction of label 1, skill, batch sizes cycled over the rows, kind)
CASES = {
    "n1": (1, 1.0, 1.0, (1,), "plain"),
    "n2": (2, 0.5, 1.0, (2,), "plain"),
    "n63": (63, 0.3, 1.0, (16,), "plain"),
    "n64": (64, 0.7, 0.5, (64,), "plain"),
    "n65": (65, 0.2, 1.5, (8,), "plain"),
    "n257": (257, 0.35, 0.8, (32,), "plain"),
    "n513": (513, 0.6, 0.3, (100,), "plain"),
    "n1031": (1031, 0.25, 1.0, (128,), "plain"),
    "all_real": (40, 0.0, 1.0, (16,), "all_real"),
    "all_fake": (40, 1.0, 0.0, (16,), "plain"),
    "all_wrong": (48, 0.4, 1.0, (16,), "all_wrong"),
    "unlabelled": (90, 0.4, 1.0, (16,), "unlabelled"),
    "argmax_tie": (50, 0.5, 0.7, (16,), "argmax_tie"),
    "mixed_batches": (111, 0.45, 0.9, (1, 3, 32), "plain"),
}
TRAIN_EPOCH_CASE = "mixed_batches"
CE_WEIGHT = [0.7, 1.3]


def make_labels(rng, n, frac):
    k = int(round(frac * n))
    y = np.zeros(n, dtype=np.int64)
    y[rng.permutation(n)[:k]] = 1
    return y


def make_logits(rng, labels, skill, kind="plain", tie_frac=1.0 / 3.0):
    """(n, 2) fp32 logits: about ``tie_frac`` of the rows repeat another row's logits bit for bit, the others take
    distinct probabilities of GRID, ranked by ``skill * (2 y - 1) + noise``"""
    n = len(labels)
    n_tie = int(n * tie_frac) if n > 2 else 0
    n_dist = n - n_tie
    rows = rng.permutation(n)
    dist, ties = rows[:n_dist], rows[n_dist:]
    sign = 2.0 * labels[dist] - 1.0
    score = skill * sign + rng.normal(size=n_dist)
    if kind == "all_wrong":
        p = np.where(sign > 0, rng.permutation(GRID[GRID < 0.45])[:n_dist], rng.permutation(GRID[GRID > 0.55])[:n_dist])
    elif kind == "all_real":
        p = rng.permutation(GRID[GRID < 0.45])[:n_dist]
    else:
        p = np.sort(rng.choice(GRID, size=n_dist, replace=False))[np.argsort(np.argsort(score))]
    z = np.zeros((n, 2), dtype=np.float32)
    z[dist, 0] = rng.uniform(-2.0, 2.0, size=n_dist).astype(np.float32)
    z[dist, 1] = (z[dist, 0].astype(np.float64) + np.log(p / (1.0 - p))).astype(np.float32)
    if kind == "argmax_tie":
        z[dist[::5], 1] = z[dist[::5], 0]
    src = rng.choice(dist, size=len(ties))
    if kind == "all_wrong":  # a tied row repeats a row of its own class, so it is wrong too
        src = np.array([rng.choice(dist[labels[dist] == labels[t]]) for t in ties], dtype=np.int64)
    z[ties] = z[src]
    return z


def softmax_fake(z):
    return torch.softmax(torch.from_numpy(z), dim=1)[:, 1].numpy()


def assert_separated(name, z, tie_case=False):
    p = softmax_fake(z).astype(np.float64)
    d = z[:, 1].astype(np.float64) - z[:, 0].astype(np.float64)
    assert np.abs(d).max() <= 8.0, name
    eq = z[:, 1] == z[:, 0]
    assert tie_case or not eq.any(), name
    assert not tie_case or (eq.sum() >= 3 and (p[eq] == 0.5).all()), name
    free = ~eq
    assert np.abs(p[free, None] - THRESHOLDS[None, :].astype(np.float64)).min() >= 1e-4, name
    order = np.argsort(p, kind="stable")
    ps, zs, es = p[order], z[order], eq[order]
    close = np.nonzero(np.diff(ps) < 1e-5)[0]
    for k in close:  # two argmax-tie rows are both 0.5 exactly
        assert (zs[k] == zs[k + 1]).all() or (es[k] and es[k + 1]), (name, ps[k], ps[k + 1])
    n_tied = len(z) - len(np.unique(z, axis=0))
    assert len(z) <= 2 or n_tied >= len(z) // 4, (name, n_tied)


def split(n, sizes):
    out, i = [], 0
    while n > 0:
        b = min(sizes[i % len(sizes)], n)
        out.append(b)
        n -= b
        i += 1
    return out


class Stub(torch.nn.Module):
    """the reference trainer's model: has ``models`` (so the trainer unpacks a tuple), one dummy parameter, and
    returns the next canned logits"""

    def __init__(self, calls):
        super().__init__()
        self.models = torch.nn.ModuleList()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls, self.i = calls, 0

    def forward(self, images):
        z = self.calls[self.i]
        self.i += 1
        assert z.shape[0] == images.shape[0]
        return z + 0.0 * self.w, None


class Recording(torch.nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.ce = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
        self.losses = []

    def forward(self, z, y):
        loss = self.ce(z, y)
        self.losses.append(loss.item())
        return loss


def batches_of(z, y, sizes, as_dict=False):
    """(loader, canned logits per call): the loader is a list of batches, images a (B, 1) dummy"""
    loader, calls, o = [], [], 0
    for b in sizes:
        x, yy = torch.zeros(b, 1), torch.from_numpy(y[o:o + b])
        loader.append({"frames": x, "label": yy} if as_dict else (x, yy))
        calls.append(torch.from_numpy(z[o:o + b]))
        o += b
    return loader, calls


def weighted_prf(y, pred):
    from sklearn.metrics import precision_recall_fscore_support

    p, r, f, _ = precision_recall_fscore_support(y, pred, average="weighted", zero_division=0)
    return {"precision": float(p), "recall": float(r), "f1": float(f)}


def main():
    ref = sys.argv[1]
    sys.path.insert(0, os.path.join(ref, "src"))
    from ensemble_trainer import EnsembleTrainer  # noqa: E402

    arrays, results = {}, {"cases": {}, "thresholds": [float(t) for t in THRESHOLDS]}
    for ci, (name, (n, frac, skill, sizes, kind)) in enumerate(CASES.items()):
        rng = np.random.default_rng(1000 + ci)
        y = make_labels(rng, n, frac)
        z = make_logits(rng, y, skill, kind)
        assert_separated(name, z, tie_case=kind == "argmax_tie")
        full_y = y.copy()
        if kind == "unlabelled":
            full_y[1::3] = -1
        bs = split(n, sizes)
        # the reference sees the labelled rows only (the mask of src/train.py:223), batch by batch
        keep = full_y >= 0
        loader, calls, o = [], [], 0
        for b in bs:
            k = keep[o:o + b]
            assert k.any()
            loader.append((torch.zeros(int(k.sum()), 1), torch.from_numpy(full_y[o:o + b][k])))
            calls.append(torch.from_numpy(z[o:o + b][k]))
            o += b
        with tempfile.TemporaryDirectory() as td:
            tr = EnsembleTrainer(Stub(calls), device="cpu", checkpoint_dir=td)
            crit = Recording(CE_WEIGHT)
            m = tr.validate(loader, crit, 1)
            assert kind != "all_wrong" or m["accuracy"] == 0.0
            rec = {"validate": m, "weighted": weighted_prf(full_y[keep], (z[keep, 1] > z[keep, 0]).astype(int))}
            arrays[f"{name}/losses"] = np.asarray(crit.losses, dtype=np.float64)
            if name == TRAIN_EPOCH_CASE:
                tr = EnsembleTrainer(Stub(calls), device="cpu", checkpoint_dir=td)
                opt, _ = tr.prepare_optimizers()
                rec["train_epoch"] = tr.train_epoch(loader, opt, Recording(CE_WEIGHT), 1)
                rec["train_epoch"] = {k: float(v) for k, v in rec["train_epoch"].items()}
        results["cases"][name] = rec
        arrays[f"{name}/logits"], arrays[f"{name}/labels"] = z, full_y
        arrays[f"{name}/batches"] = np.asarray(bs, dtype=np.int64)
        arrays[f"{name}/probs"] = softmax_fake(z)
        print(name, {k: v for k, v in m.items() if k != "confusion_matrix"}, m["confusion_matrix"])

    # ---- the epoch loop: 12 epochs over three train() calls on one trainer
    rng = np.random.default_rng(7)
    n_epochs = 12
    ty, vy = make_labels(rng, 11, 0.36), make_labels(rng, 24, 0.42)
    t_sizes, v_sizes = [4, 4, 3], [10, 10, 4]
    # validation skill per epoch: improves, regresses at 3-4 and 8, plateaus
    v_skill = [0.0, 0.6, 0.3, 0.2, 1.2, 0.4, 0.9, 0.1, 1.6, 1.0, 2.2, 0.5]
    tz = np.stack([make_logits(rng, ty, 0.2 * e) for e in range(n_epochs)])
    vz = np.stack([make_logits(rng, vy, v_skill[e]) for e in range(n_epochs)])
    for e in range(n_epochs):
        assert_separated(f"run/train{e}", tz[e])
        assert_separated(f"run/val{e}", vz[e])
    calls = []
    for e in range(n_epochs):
        calls += batches_of(tz[e], ty, t_sizes)[1] + batches_of(vz[e], vy, v_sizes)[1]
    train_loader = batches_of(tz[0], ty, t_sizes)[0]
    val_loader = batches_of(vz[0], vy, v_sizes, as_dict=True)[0]
    plan = [dict(epochs=5, start_epoch=1, class_weights=None, select_metric="f1_thr"),
            dict(epochs=11, start_epoch=6, class_weights=[0.8, 1.25], select_metric="acc"),
            dict(epochs=12, start_epoch=12, class_weights=[0.8, 1.25], select_metric="no_such_metric")]
    run = {"plan": plan, "after": []}
    with tempfile.TemporaryDirectory() as td:
        tr = EnsembleTrainer(Stub(calls), device="cpu", checkpoint_dir=td)
        for kw in plan:
            kw = dict(kw)
            cw = kw.pop("class_weights")
            tr.train(train_loader, val_loader, lr=1e-3, weight_decay=1e-5,
                     class_weights=None if cw is None else torch.tensor(cw), **kw)
            run["after"].append({
                "history_csv": open(os.path.join(td, "training_history.csv"), newline="").read(),
                "calibration": json.load(open(os.path.join(td, "calibration_best.json"))),
                "best_metrics": dict(tr.best_metrics),
                "files": sorted(os.listdir(td)),
            })
            print(kw, tr.best_metrics, run["after"][-1]["files"])
        run["history"] = tr.training_history
        assert tr.model.i == len(calls)
    results["run"] = run
    arrays["run/train_labels"], arrays["run/val_labels"] = ty, vy
    arrays["run/train_logits"], arrays["run/val_logits"] = tz, vz
    arrays["run/train_batches"] = np.asarray(t_sizes, dtype=np.int64)
    arrays["run/val_batches"] = np.asarray(v_sizes, dtype=np.int64)

    path = os.path.join(HERE, "epoch_metrics.npz")
    np.savez_compressed(path, **arrays)
    jpath = os.path.join(HERE, "epoch_metrics.json")
    with open(jpath, "w") as f:
        json.dump(results, f, indent=1, default=float)
    print(f"{len(arrays)} arrays, {os.path.getsize(path)} + {os.path.getsize(jpath)} bytes -> {path}, {jpath}")


if __name__ == "__main__":
    main()
