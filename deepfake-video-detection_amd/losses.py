"""Weighted cross entropy on HIP -- drop-in for ``nn.CrossEntropyLoss(weight=...)``.

Reference uses: ``criterion = nn.CrossEntropyLoss(weight=class_weights)``
(``src/ensemble_trainer.py:358``, ``src/train.py:337``) on ``(B, 2)`` logits, mean reduction:
``sum_b w[y_b] * (-log softmax(z_b)[y_b]) / sum_b w[y_b]``.  Forward and backward are one HIP
kernel each (``torch.ops.dfd.weighted_cross_entropy``, autograd registered on the op) and never
synchronise with the host.

``FocalLoss`` and ``SmoothedCrossEntropyLoss`` are the two criteria of the reference's ``ImprovedTrainer``
(``src/train_improved.py:29-78`` and ``:136-150``: ``FocalLoss(gamma, weight, label_smoothing)`` or
``nn.CrossEntropyLoss(weight, label_smoothing)``) on ``(B, C)`` logits, ``1 <= C <= 1024``, with the
reductions ``mean`` / ``sum`` / ``none`` (``torch.ops.dfd.classification_loss``, ``csrc/k_loss.hip``).  A label
outside ``[0, C)`` gives that row a NaN loss and a zero gradient instead of an out-of-range read.  As in the
reference, ``FocalLoss`` with ``0 < gamma < 1`` is undefined (inf / NaN gradients) on a row whose ``pt``
rounds to 1.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, ops  # noqa: F401  (registers torch.ops.dfd.*)


class WeightedCrossEntropyLoss(nn.Module):
    def __init__(self, weight: torch.Tensor | None = None, ignore_index: int = -100, reduction: str = "mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("only reduction='mean' (the reference's setting) is implemented")
        self.register_buffer("weight", None if weight is None else weight.detach().float().clone())
        self.ignore_index = ignore_index

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        _lib.require_hip(logits, "logits")
        if self.weight is not None and (self.weight.device != logits.device or not self.weight.is_contiguous()):
            # moved once: a per-step host->device copy of a pageable tensor blocks the host until the
            # queue drains (measured 7 ms/step of host stall in the bench step, tools/host_prof.py)
            self.weight = self.weight.to(logits.device).contiguous()
        w = self.weight
        loss, _ = torch.ops.dfd.weighted_cross_entropy(logits, target, w, self.ignore_index)
        return loss


def _weight_buffer(weight):
    """the reference's constructor contract (train_improved.py:40-46): a tensor, None, or a list / tuple"""
    if weight is None:
        return None
    if not isinstance(weight, torch.Tensor):
        weight = torch.tensor(weight, dtype=torch.float32)
    return weight.detach().to(dtype=torch.float32).clone()


class _ClassificationLoss(nn.Module):
    mode = ""

    def __init__(self, weight, label_smoothing, reduction):
        super().__init__()
        if reduction not in ops.LOSS_REDUCTIONS:
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none' (got {reduction!r})")
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1) (got {label_smoothing})")
        self.register_buffer("weight", _weight_buffer(weight))
        self.label_smoothing = float(label_smoothing)
        self.reduction = reduction
        self.gamma = 0.0
        self.ignore_index = -100

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        _lib.require_hip(logits, "logits")
        _lib.require_hip(target, "target")
        if logits.dim() != 2 or target.shape != logits.shape[:1]:
            raise ValueError(f"expected logits (B, C) and target (B,), got {tuple(logits.shape)}, {tuple(target.shape)}")
        w = self.weight
        if w is not None and w.numel() != logits.shape[1]:
            raise ValueError(f"weight has {w.numel()} entries for {logits.shape[1]} classes")
        if w is not None and (w.device != logits.device or not w.is_contiguous()):
            self.weight = w = w.to(logits.device).contiguous()  # moved once (see WeightedCrossEntropyLoss)
        loss, _ = torch.ops.dfd.classification_loss(logits, target, w, self.mode, self.reduction, float(self.gamma),
                                                    self.label_smoothing, self.ignore_index)
        return loss


class FocalLoss(_ClassificationLoss):
    """``FocalLoss`` of ``src/train_improved.py:29-78``: ``w[y] (1 - pt)^gamma L`` with the smoothed target
    distribution; ``mean`` is the plain mean over the batch."""

    mode = "focal"

    def __init__(self, gamma=2.0, weight=None, label_smoothing=0.0, reduction="mean"):
        super().__init__(weight, label_smoothing, reduction)
        self.gamma = gamma


class SmoothedCrossEntropyLoss(_ClassificationLoss):
    """``nn.CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing)`` for class-index targets."""

    mode = "ce"

    def __init__(self, weight=None, label_smoothing=0.0, ignore_index=-100, reduction="mean"):
        super().__init__(weight, label_smoothing, reduction)
        self.ignore_index = int(ignore_index)
