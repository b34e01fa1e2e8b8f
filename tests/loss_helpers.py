"""The two criteria of the ViT+GCN trainer restated in plain torch, and the grid their tests share.

``focal_loss`` / ``smoothed_ce`` restate ``FocalLoss`` (``src/train_improved.py:29-78``) and torch's
``cross_entropy(weight, label_smoothing, ignore_index)`` in closed form on the label's entry and the row sums
(no dense target distribution, no ``log_softmax``), in the dtype of the logits -- fp64 for the oracle of the GPU
tests.  ``tests/golden/improved_losses.npz`` (``make_improved_golden.py``) holds what the reference's own
``FocalLoss`` and ``nn.CrossEntropyLoss`` give on the same grid in fp32; ``test_losses_host.py`` holds the
restatement to it.

Grid.  Shapes (B, C): (1, 2) smallest B; (5, 2) a partial workgroup (4 rows per workgroup); (67, 3) odd C, a
partial last workgroup; (300, 2) 75 workgroups and more rows than the reduction's 256 threads; (33, 65) one
more class than lanes; (4, 1) the C == 1 smoothing branch.  gamma 0 / 0.5 / 2 / 3.5, label smoothing 0 / 0.1,
weights none / ones / inverse frequency, and for the cross entropy the targets plain, with ignored rows
(``ign``, B >= 4) and with every row but one ignored (``one``; (5, 2) and (67, 3)).  Logits are N(0, 2^2).

Left out: gamma = 0.5 at (4, 1) without smoothing.  With one class and eps = 0, pt is exactly 1 on every row,
which is the documented undefined region (0 < gamma < 1 at pt = 1: the reference's own gradient is NaN there).
"""
from __future__ import annotations

import itertools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "improved_losses.npz")
SHAPES = [(1, 2), (5, 2), (67, 3), (300, 2), (33, 65), (4, 1)]
GAMMAS = [0.0, 0.5, 2.0, 3.5]
EPS = [0.0, 0.1]
WEIGHTS = ["none", "ones", "invfreq"]
REDUCTIONS = ["mean", "sum", "none"]
IGNORE = -100
SEED = 1234


def shape_inputs(B, C):
    """(logits (B, C) fp32 ~ N(0, 2^2), targets (B,) int64), fixed per shape"""
    g = torch.Generator().manual_seed(SEED + 1000 * B + C)
    return torch.randn(B, C, generator=g) * 2.0, torch.randint(0, C, (B,), generator=g)


def class_weight(kind, targets, C):
    if kind == "none":
        return None
    if kind == "ones":
        return torch.ones(C)
    count = torch.bincount(targets[targets >= 0], minlength=C).clamp(min=1).float()
    return float(targets.numel()) / (C * count)


def ce_targets(kind, targets):
    """'plain'; 'ign': every third row ignored, starting with row 1; 'one': every row but row 2 ignored"""
    t = targets.clone()
    if kind == "ign":
        t[1::3] = IGNORE
    elif kind == "one":
        keep = t[2].item()
        t[:] = IGNORE
        t[2] = keep
    return t


def focal_cases(shapes=None):
    for (B, C), gamma, eps, wk in itertools.product(shapes or SHAPES, GAMMAS, EPS, WEIGHTS):
        if C == 1 and eps == 0.0 and 0.0 < gamma < 1.0:
            continue  # pt == 1 on every row: undefined (module docstring)
        yield B, C, gamma, eps, wk


def ce_cases(shapes=None):
    for (B, C), eps, wk in itertools.product(shapes or SHAPES, EPS, WEIGHTS):
        yield B, C, eps, wk, "plain"
        if B >= 4:
            yield B, C, eps, wk, "ign"
        if (B, C) in ((5, 2), (67, 3)):
            yield B, C, eps, wk, "one"


def focal_key(B, C, gamma, eps, wk):
    return f"focal/{B}x{C}/g{gamma}/e{eps}/{wk}"


def ce_key(B, C, eps, wk, tk):
    return f"ce/{B}x{C}/e{eps}/{wk}/{tk}"


def _reduce(rows, reduction, denom):
    if reduction == "mean":
        return rows.sum() / denom
    return rows.sum() if reduction == "sum" else rows


def focal_loss(logits, targets, gamma, weight=None, eps=0.0, reduction="mean"):
    B, C = logits.shape
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    lp_y = logp.gather(1, targets[:, None]).squeeze(1)
    p_y = lp_y.exp()
    off = eps / (C - 1) if C > 1 else 0.0
    # q = off everywhere, 1 - eps at the label
    L = -((1.0 - eps) * lp_y + off * (logp.sum(dim=1) - lp_y))
    pt = (1.0 - eps) * p_y + off * (logp.exp().sum(dim=1) - p_y)
    rows = (1.0 - pt) ** gamma * L
    if weight is not None:
        rows = rows * weight.to(logits)[targets]
    return _reduce(rows, reduction, B)


def focal_pt(logits, targets, eps):
    """pt = sum_c q_c p_c per row, with the dense target distribution"""
    C = logits.shape[1]
    q = torch.full_like(logits, eps / (C - 1) if C > 1 else 0.0)
    q.scatter_(1, targets[:, None], 1.0 - eps)
    return (q * torch.softmax(logits, dim=1)).sum(dim=1)


def smoothed_ce(logits, targets, weight=None, eps=0.0, ignore_index=IGNORE, reduction="mean"):
    B, C = logits.shape
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    keep = targets != ignore_index
    t = torch.where(keep, targets, torch.zeros_like(targets))
    w = torch.ones(C, dtype=logits.dtype, device=logits.device) if weight is None else weight.to(logits)
    wy = w[t] * keep
    nll = -logp.gather(1, t[:, None]).squeeze(1)
    rows = (1.0 - eps) * wy * nll - (eps / C) * (logp * w).sum(dim=1) * keep
    return _reduce(rows, reduction, wy.sum())


def with_grad(fn, logits, *args, upstream=None, **kw):
    """(loss, dlogits) of a criterion; ``upstream``: the gradient of the output (default ones)"""
    z = logits.detach().clone().requires_grad_(True)
    out = fn(z, *args, **kw)
    out.backward(torch.ones_like(out) if upstream is None else upstream.to(out))
    return out.detach(), z.grad.detach()


FIELDS = ("rows", "mean", "sum", "dmean")


def case_groups():
    """{'focal/BxC' or 'ce/BxC': [case keys in grid order]}: the fixture stacks a group's cases per field"""
    groups = {}
    for c in focal_cases():
        groups.setdefault(f"focal/{c[0]}x{c[1]}", []).append(focal_key(*c))
    for c in ce_cases():
        groups.setdefault(f"ce/{c[0]}x{c[1]}", []).append(ce_key(*c))
    return groups


def load_golden():
    """{'in/BxC/logits' | 'in/BxC/targets' | '<case key>/<field>': tensor}"""
    out = {}
    with np.load(GOLDEN) as f:
        stacked = {f"{g}/{fld}": keys for g, keys in case_groups().items() for fld in FIELDS}
        for name in f.files:
            arr = torch.from_numpy(f[name])
            if name in stacked:
                for i, k in enumerate(stacked[name]):
                    out[f"{k}/{name.rsplit('/', 1)[1]}"] = arr[i]
            else:
                out[name] = arr
    return out
