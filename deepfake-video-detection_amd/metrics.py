"""Per-epoch metrics of a binary (2-logit) classifier, accumulated on the device.

The reference's ``EnsembleTrainer.train_epoch`` / ``validate`` (``src/ensemble_trainer.py:203-211, 266-273``) read
``loss.item()`` and three ``.cpu()`` copies after every step and hand the lists to sklearn at the end of the epoch
(``:276-329``).  ``EpochMetrics`` keeps the scores on the device instead: ``update`` is one ``dfd::metrics_append``
launch and never synchronises, ``compute`` runs ``dfd::metrics_finalize`` (integer counts and the exact Mann-Whitney
pair count, ``csrc/k_metrics.hip``) and reads one small block back -- the epoch's single host sync.  The arithmetic
on those integers is ``metrics_from_counts``, a pure host function (no device, no sklearn) that reproduces the
reference's numbers including its corner cases.

The accumulator sees the rows of one process: gathering the shards of ``DataParallelTrainer`` ranks is out of scope
(the reference has no data parallelism).
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib, ops

# the threshold grid of the reference's sweep (ensemble_trainer.py:304), as fp32 values
SWEEP_THRESHOLDS = np.linspace(0.05, 0.95, 19, dtype=np.float32)
TAG_LABEL, TAG_PRED, TAG_VALID = 1, 2, 4  # include/dfd_hip.h: DFD_METRICS_TAG_*


def _div0(num: float, den: float) -> float:
    """sklearn's ``zero_division=0``"""
    return float(num) / float(den) if den else 0.0


def metrics_from_counts(n_pos: int, n_neg: int, tn: int, fp: int, fn: int, tp: int, u2: int,
                        thresholds: Sequence[float] = (), tp_t: Sequence[int] = (), fp_t: Sequence[int] = (),
                        loss: float = 0.0, average: str = "binary") -> dict:
    """The metric dict of ``EnsembleTrainer.validate`` (``src/ensemble_trainer.py:276-329``) from integer counts.

    ``tn, fp, fn, tp``: the confusion counts of the argmax predictions over the labelled rows; ``u2`` = the sum over
    (positive i, negative j) of ``2 [p_i > p_j] + [p_i == p_j]``; ``tp_t[k]`` / ``fp_t[k]``: the true / false
    positives of ``prob >= thresholds[k]``.  As in the reference:

    * precision, recall and F1 are 0.0 where their denominator is 0 (``zero_division=0``);
    * ``auc`` is 0.5 with one class present, and the four sweep keys are then absent;
    * the sweep keeps the first threshold whose score is strictly greater;
    * ``confusion_matrix`` is over the sorted union of the labels seen in truth and prediction (all-real truth and
      prediction: ``[[N]]``); with no labelled row it is ``[]`` and every metric 0.0 (sklearn raises there).

    ``average='weighted'``: the support-weighted precision / recall / F1 of ``ImprovedTrainer``
    (``src/train_improved.py:222-224``) instead of the fake class's."""
    if average not in ("binary", "weighted"):
        raise ValueError(f"average must be 'binary' or 'weighted' (got {average!r})")
    n_pos, n_neg, tn, fp, fn, tp, u2 = (int(v) for v in (n_pos, n_neg, tn, fp, fn, tp, u2))
    if tp + fn != n_pos or tn + fp != n_neg:
        raise ValueError("confusion counts do not add up to the class counts")
    n = n_pos + n_neg
    # per class: (true positives, predicted, support)
    per_class = ((tn, tn + fn, n_neg), (tp, tp + fp, n_pos))
    prf = [(_div0(t, pred), _div0(t, sup), _div0(2 * t, pred + sup)) for t, pred, sup in per_class]
    if average == "binary":
        precision, recall, f1 = prf[1]
    else:
        precision, recall, f1 = (_div0(n_neg * prf[0][k] + n_pos * prf[1][k], n) for k in range(3))
    both = n_pos > 0 and n_neg > 0
    seen0, seen1 = n_neg > 0 or tn + fn > 0, n_pos > 0 or tp + fp > 0
    if seen0 and seen1:
        cm = [[tn, fp], [fn, tp]]
    elif seen0 or seen1:
        cm = [[n]]
    else:
        cm = []
    out = {
        "loss": float(loss),
        "accuracy": _div0(tp + tn, n),
        "precision": precision,
        "recall": recall,
        "f1": f1,
        "auc": u2 / (2.0 * n_pos * n_neg) if both else 0.5,
        "confusion_matrix": cm,
    }
    if both and len(thresholds):
        best_acc, best_thr_acc, best_f1, best_thr_f1 = -1.0, 0.5, -1.0, 0.5
        for thr, tpk, fpk in zip(thresholds, tp_t, fp_t):
            tpk, fpk = int(tpk), int(fpk)
            acc = (tpk + (n_neg - fpk)) / n
            f1k = _div0(2 * tpk, tpk + fpk + n_pos)
            if acc > best_acc:
                best_acc, best_thr_acc = acc, float(thr)
            if f1k > best_f1:
                best_f1, best_thr_f1 = f1k, float(thr)
        out["best_thr_accuracy"] = best_thr_acc
        out["accuracy_thr"] = best_acc
        out["best_thr_f1"] = best_thr_f1
        out["f1_thr"] = best_f1
    return out


class EpochMetrics:
    """``update`` after every step, ``compute`` once per epoch, ``reset`` before the next one.

    State on ``device``: the fake-class probability (fp32) and a tag byte (label, argmax prediction, labelled) per
    row, and two fp64 loss sums.  The row count lives on the host (batch sizes are shapes), so an update needs no
    read-back; rows whose label is not 0 / 1 (``-1``: unlabelled, ``src/train.py:223``) are stored and skipped by
    the finalize."""

    def __init__(self, device, capacity: int = 4096):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DFDError(f"EpochMetrics lives on a HIP device (got {self.device}); there is no CPU fallback")
        self._alloc(max(int(capacity), 1))
        self._sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.n = 0  # rows appended this epoch
        self.batches = 0  # updates that carried a loss

    def _alloc(self, capacity: int) -> None:
        self._probs = torch.empty(capacity, dtype=torch.float32, device=self.device)
        self._tags = torch.empty(capacity, dtype=torch.uint8, device=self.device)

    @property
    def capacity(self) -> int:
        return self._probs.numel()

    def _grow(self, need: int) -> None:
        old_p, old_t = self._probs, self._tags
        self._alloc(max(2 * self.capacity, need))
        self._probs[:self.n].copy_(old_p[:self.n], non_blocking=True)  # device to device, in stream order
        self._tags[:self.n].copy_(old_t[:self.n], non_blocking=True)

    def update(self, logits: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor | None = None) -> None:
        """logits (B, 2) and int64 labels (B) on the device, ``loss`` a device scalar (the step's mean loss)."""
        if logits.dim() != 2 or logits.shape[1] != 2:
            raise ValueError(f"EpochMetrics is binary: logits must be (B, 2), got {tuple(logits.shape)}")
        _lib.require_hip(logits, "logits")
        B = int(logits.shape[0])
        if B == 0:
            return
        if self.n + B > self.capacity:
            self._grow(self.n + B)
        labels = labels.to(self.device, non_blocking=True)
        torch.ops.dfd.metrics_append(logits.detach(), labels, None if loss is None else loss.detach(), self.n,
                                     self._probs, self._tags, self._sums)
        self.n += B
        self.batches += loss is not None

    def reset(self) -> None:
        """a new epoch; the buffers are kept (rows past ``n`` are never read)"""
        self.n = 0
        self.batches = 0
        self._sums.zero_()

    def probs(self) -> torch.Tensor:
        """device view of this epoch's fake-class probabilities, in append order (unlabelled rows included)"""
        return self._probs[:self.n]

    def tags(self) -> torch.Tensor:
        return self._tags[:self.n]

    def labels(self) -> torch.Tensor:
        """this epoch's labels on the device, int64; -1 for an unlabelled row"""
        t = self.tags().long()
        return torch.where((t & TAG_VALID) != 0, t & TAG_LABEL, torch.full_like(t, -1))

    def preds(self) -> torch.Tensor:
        return (self.tags().long() & TAG_PRED) >> 1

    def counts(self, thresholds=None) -> dict:
        """Finalize and read back: the integer counts, the thresholds (fp32 values) and the two loss sums."""
        thr = SWEEP_THRESHOLDS if thresholds is None else np.asarray(thresholds, dtype=np.float32).reshape(-1)
        if len(thr) > ops.METRICS_MAX_THRESHOLDS:
            raise ValueError(f"at most {ops.METRICS_MAX_THRESHOLDS} thresholds (got {len(thr)})")
        res = torch.ops.dfd.metrics_finalize(self._probs, self._tags, self.n, [float(t) for t in thr])
        # one copy, one synchronisation: the result block and the loss sums (bit patterns) together
        host = torch.cat([res, self._sums.view(torch.int64)]).cpu().numpy()
        r, sums = host[:ops.METRICS_RESULT_WORDS], host[ops.METRICS_RESULT_WORDS:].view(np.float64)
        k = len(thr)
        return {"n_pos": int(r[0]), "n_neg": int(r[1]), "tn": int(r[2]), "fp": int(r[3]), "fn": int(r[4]),
                "tp": int(r[5]), "u2": int(r[6].view(np.uint64)), "thresholds": [float(t) for t in thr],
                "tp_t": [int(v) for v in r[8:8 + k]], "fp_t": [int(v) for v in r[40:40 + k]],
                "loss_sum": float(sums[0]), "loss_weighted_sum": float(sums[1])}

    def compute(self, average: str = "binary", thresholds=None, loss_mean: str = "per_batch") -> dict:
        """The reference's metric dict for the rows appended since ``reset`` (keys and corner cases:
        ``metrics_from_counts``).  ``loss_mean='per_batch'``: the sum of the step losses over the number of steps
        (``ensemble_trainer.py:223``); ``'per_sample'``: ``sum(loss * B) / sum(B)`` (``train.py:128,133``)."""
        if loss_mean not in ("per_batch", "per_sample"):
            raise ValueError(f"loss_mean must be 'per_batch' or 'per_sample' (got {loss_mean!r})")
        c = self.counts(thresholds)
        if loss_mean == "per_batch":
            loss = c["loss_sum"] / self.batches if self.batches else 0.0
        else:
            loss = c["loss_weighted_sum"] / self.n if self.n else 0.0
        return metrics_from_counts(c["n_pos"], c["n_neg"], c["tn"], c["fp"], c["fn"], c["tp"], c["u2"],
                                   c["thresholds"], c["tp_t"], c["fp_t"], loss=loss, average=average)
