"""Golden fixture for the ViT+GCN trainer's criteria: ``improved_losses.npz``.

Runs the REFERENCE ``FocalLoss`` (``src/train_improved.py:29-78``, imported from a checkout of the reference;
development machine only) and torch's ``nn.CrossEntropyLoss(weight, label_smoothing)`` (the other criterion of
``ImprovedTrainer``, ``:136-150``) on the CPU in fp32 over the grid of ``tests/loss_helpers.py`` and records, per
shape, the logits and targets and, per case, the per-row losses, the ``mean`` and ``sum`` losses and ``dlogits``
of the ``mean`` loss -- plus a saturated batch (logit gap 40) for the focal loss at gamma 0 and 2.

    python tests/golden/make_improved_golden.py /path/to/reference
"""
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loss_helpers as lh  # noqa: E402


def saturated():
    """(6, 2) logits +-20 (gap 40); rows 0-3 labelled with the winning class (pt rounds to 1), 4-5 with the other"""
    z = torch.tensor([[20.0, -20.0], [-20.0, 20.0]]).repeat(3, 1)
    t = torch.tensor([0, 1, 0, 1, 1, 0])
    return z, t


def main():
    ref = sys.argv[1]
    for name in ("tqdm", "cv2", "timm"):  # imported at module level by the reference, unused by FocalLoss
        try:
            importlib.import_module(name)
        except ImportError:
            stub = types.ModuleType(name)
            stub.tqdm = lambda it, **kw: it
            sys.modules[name] = stub
    sys.path.insert(0, os.path.join(ref, "src"))
    from train_improved import FocalLoss  # noqa: E402

    out = {}

    def record(key, make, z, t):
        for red in ("mean", "sum", "none"):
            loss, dz = lh.with_grad(lambda x: make(red)(x, t), z)
            out[f"{key}/{'rows' if red == 'none' else red}"] = loss.numpy()
            if red == "mean":
                out[f"{key}/dmean"] = dz.numpy()

    for B, C in lh.SHAPES:
        z, t = lh.shape_inputs(B, C)
        out[f"in/{B}x{C}/logits"], out[f"in/{B}x{C}/targets"] = z.numpy(), t.numpy()
    for B, C, gamma, eps, wk in lh.focal_cases():
        z, t = lh.shape_inputs(B, C)
        w = lh.class_weight(wk, t, C)
        record(lh.focal_key(B, C, gamma, eps, wk),
               lambda red: FocalLoss(gamma=gamma, weight=w, label_smoothing=eps, reduction=red), z, t)
    for B, C, eps, wk, tk in lh.ce_cases():
        z, t = lh.shape_inputs(B, C)
        w = lh.class_weight(wk, t, C)
        record(lh.ce_key(B, C, eps, wk, tk),
               lambda red: torch.nn.CrossEntropyLoss(weight=w, label_smoothing=eps, ignore_index=lh.IGNORE,
                                                     reduction=red), z, lh.ce_targets(tk, t))
    z, t = saturated()
    out["in/sat/logits"], out["in/sat/targets"] = z.numpy(), t.numpy()
    for gamma in (0.0, 2.0):
        record(f"focal/sat/g{gamma}", lambda red: FocalLoss(gamma=gamma, reduction=red), z, t)
    for group, keys in lh.case_groups().items():  # one stacked array per shape and field
        for fld in lh.FIELDS:
            out[f"{group}/{fld}"] = np.stack([out.pop(f"{k}/{fld}") for k in keys])
    path = os.path.join(HERE, "improved_losses.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
