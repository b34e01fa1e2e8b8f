"""Train-step API: the reference's ``EnsembleTrainer.train_epoch`` step on HIP, single- and multi-GPU.

Reference step (``src/ensemble_trainer.py:182-203``)::

    optimizer.zero_grad(); outputs = model(images); loss = criterion(outputs, labels)
    loss.backward(); clip_grad_norm_(model.parameters(), 1.0); optimizer.step(); loss.item()

``TrainStep`` runs exactly that with the HIP detector, the HIP weighted cross entropy and the
fused clip+AdamW kernel, without the per-step host sync: the step returns the loss as a device
scalar.  ``EnsembleTrainer`` (below) is the reference's whole trainer around that step -- epoch loop,
validation, metrics, best-checkpoint selection, ``training_history.csv``, ``calibration_best.json`` --
with the per-step bookkeeping kept on the device (``metrics.EpochMetrics``): one host sync per epoch
pass instead of four per step.  ``DataParallelTrainer`` shards clips across ranks (one process per GPU,
``torch.distributed`` / RCCL over xGMI): gradients are summed by bucketed async all-reduce
launched from inside backward as soon as a segment's gradients are enqueued (reverse network
order: head, conv_head, stage 6, 5, ...), so communication overlaps the remaining backward
(RCCL runs on its own stream); the loss is pre-divided by the world size so the sum is the
mean.  BatchNorm statistics stay local per rank (the reference has no SyncBN).

With the fp16 trunk (``compute_dtype="fp16"``) the step scales the loss by a ``DynamicLossScaler``
before backward (fp16 activation gradients would underflow) and the fused optimizer unscales, skips
non-finite steps and updates the scale on the device (``torch.amp.GradScaler`` semantics, no sync).

``ImprovedTrainStep`` is the step of the reference's ``ImprovedTrainer`` (``src/train_improved.py:104-232``),
the trainer of ``DeepfakeModel`` (ViT-B/16 + SimpleGCN)::

    optimizer.zero_grad(); logits = model(frames, A_norm); loss = criterion(logits, labels)
    loss.backward(); clip_grad_norm_(model.parameters(), 1.0); optimizer.step()

with ``FocalLoss`` or the label-smoothed cross entropy on HIP, AdamW under ``CosineAnnealingLR`` stepped once
per epoch.  ``ReduceLROnPlateau``, early stopping and checkpoint naming are host bookkeeping on scalars and
stay with the caller; its per-epoch numbers (support-weighted precision / recall / F1) come from
``metrics.EpochMetrics.compute(average='weighted')``.
"""
from __future__ import annotations

import csv
import json
import logging
from pathlib import Path

import torch
import torch.distributed as dist

from . import checkpoint
from .losses import FocalLoss, SmoothedCrossEntropyLoss, WeightedCrossEntropyLoss
from .metrics import EpochMetrics
from .optim import DynamicLossScaler, FusedAdam, FusedAdamW

logger = logging.getLogger(__name__)


class TrainStep:
    def __init__(self, model, lr=1e-4, weight_decay=1e-5, class_weights=None, max_grad_norm=1.0,
                 optimizer="adamw", world_size: int = 1, criterion=None, loss_scale="auto"):
        self.model = model
        # the reference trainers hand the criterion in (ensemble_trainer.py:358 -> train_epoch); default:
        # the HIP weighted cross entropy
        self.criterion = criterion if criterion is not None else WeightedCrossEntropyLoss(weight=class_weights)
        cls = FusedAdamW if optimizer == "adamw" else FusedAdam
        self.optimizer = cls(model.parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.world_size = world_size
        # fp16 trunk: dynamic loss scaling (torch.amp.GradScaler semantics, on the device).  "auto" =
        # on when any submodule computes in fp16 (the detector, or a member of EnsembleDetector), off
        # otherwise; or a DynamicLossScaler / None.
        if loss_scale == "auto":
            fp16 = any(getattr(m, "compute_dtype", None) == "fp16" for m in model.modules())
            loss_scale = DynamicLossScaler(self.optimizer._m.device) if fp16 else None
        self.loss_scaler = loss_scale
        self.optimizer.set_loss_scaler(loss_scale)

    def forward_backward(self, images, labels):
        self.optimizer.zero_grad(set_to_none=True)
        out = self.model(images)
        logits = out[0] if isinstance(out, tuple) else out
        loss = self.criterion(logits, labels)
        l = loss / self.world_size if self.world_size > 1 else loss
        (self.loss_scaler.scale(l) if self.loss_scaler is not None else l).backward()
        return loss, logits

    def __call__(self, images, labels):
        loss, logits = self.forward_backward(images, labels)
        self.sync_grads()
        self.optimizer.step()
        return loss, logits

    def sync_grads(self):
        pass


class DataParallelTrainer(TrainStep):
    """One rank per GPU; bucketed RCCL all-reduce of the flat gradient overlapped with backward."""

    def __init__(self, model, bucket_elems: int = 1 << 20, process_group=None, **kw):
        ws = dist.get_world_size(process_group) if dist.is_initialized() else 1
        super().__init__(model, world_size=ws, **kw)
        self.pg = process_group
        self.bucket_elems = bucket_elems
        self._works = []
        self._pending = None  # (lo, hi) accumulated but not yet launched
        self._flat = None
        self.comm_enabled = True  # False: skip the exchange (bench's comm-off timing pass only)
        self.bucket_log = []  # (lo, hi) of the buckets launched by the last backward
        if ws > 1:
            self._broadcast_params()
            model.register_grad_ready_hook(self._on_ready)

    def _broadcast_params(self):
        with torch.no_grad():
            dist.broadcast(self.model._flat_p, src=0, group=self.pg)
            dist.broadcast(self.model._flat_b, src=0, group=self.pg)

    def _launch(self, flat, lo, hi):
        self.bucket_log.append((lo, hi))
        self._works.append(dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def _check_adoption(self):
        """The buckets are all-reduced in the GradSink buffer while backward runs; that is only the
        gradient if autograd ADOPTS the sink views as ``p.grad``, i.e. every ``p.grad`` is None when
        backward starts.  An existing ``.grad`` (``zero_grad(set_to_none=False)``, gradient
        accumulation) would be added to the unreduced view instead -- refuse that loudly."""
        stale = [n for n, p in self.model.named_parameters() if p.requires_grad and p.grad is not None]
        if stale:
            raise RuntimeError(
                f"DataParallelTrainer: {len(stale)} parameters (e.g. {stale[0]}) already hold a .grad at backward; "
                "the overlapped all-reduce needs zero_grad(set_to_none=True) before every backward "
                "(gradient accumulation is not supported)")

    def _on_ready(self, flat, lo, hi):
        # segments arrive in reverse order of the flat layout: merge adjacent ranges into buckets
        if not self.comm_enabled:
            return
        if self._pending is None and not self._works:  # first segment of this backward
            self._check_adoption()
            self.bucket_log = []
        self._flat = flat
        if self._pending is None:
            self._pending = (lo, hi)
        elif hi == self._pending[0]:
            self._pending = (lo, self._pending[1])
        else:
            self._launch(flat, *self._pending)
            self._pending = (lo, hi)
        if self._pending[1] - self._pending[0] >= self.bucket_elems:
            self._launch(flat, *self._pending)
            self._pending = None

    def sync_grads(self):
        if self.world_size <= 1 or not self.comm_enabled:
            return
        if self._pending is not None:
            self._launch(self._flat, *self._pending)
            self._pending = None
        for w in self._works:
            w.wait()
        self._works.clear()


class ImprovedTrainStep:
    """``ImprovedTrainer(model, device, config)``'s optimisation step.  ``config`` keys, as in the reference:
    ``learning_rate``, ``weight_decay``, ``max_epochs``, ``class_weights`` (required), ``loss`` (``'focal'`` or
    ``'cross_entropy'``, the default), ``label_smoothing`` (0), ``focal_gamma`` (2).  ``model`` is on its HIP
    device already.  Nothing in a step synchronises with the host."""

    def __init__(self, model, config):
        self.model = model
        self.config = config
        lr = float(config["learning_rate"])
        smoothing = float(config.get("label_smoothing", 0.0))
        weight = torch.as_tensor(config["class_weights"], dtype=torch.float32)
        loss_name = config.get("loss", "cross_entropy")
        if loss_name == "focal":
            self.criterion = FocalLoss(gamma=float(config.get("focal_gamma", 2.0)), weight=weight,
                                       label_smoothing=smoothing)
        elif loss_name == "cross_entropy":
            self.criterion = SmoothedCrossEntropyLoss(weight=weight, label_smoothing=smoothing)
        else:
            raise ValueError(f"config['loss'] must be 'focal' or 'cross_entropy' (got {loss_name!r})")
        if hasattr(model, "ensure_flat"):
            model.ensure_flat()
        self.optimizer = FusedAdamW(model.parameters(), lr=lr, weight_decay=float(config["weight_decay"]),
                                    betas=(0.9, 0.999), max_grad_norm=1.0)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=int(config["max_epochs"]),
                                                                    eta_min=lr * 0.01)

    def forward_backward(self, frames, A_norm, labels):
        self.optimizer.zero_grad(set_to_none=True)
        logits = self.model(frames, A_norm)
        loss = self.criterion(logits, labels)
        loss.backward()
        return loss, logits

    def __call__(self, frames, A_norm, labels):
        loss, logits = self.forward_backward(frames, A_norm, labels)
        self.optimizer.step()
        return loss, logits

    def scheduler_step(self) -> None:
        """once per epoch, after its steps (``self.scheduler.step()`` in the reference's epoch loop)"""
        self.scheduler.step()


class EnsembleTrainer:
    """The reference's ``EnsembleTrainer`` (``src/ensemble_trainer.py:103-609``): same constructor, method names,
    signatures, ``training_history`` / ``best_metrics`` and files on disk (``checkpoint_best.pt``,
    ``checkpoint_best_epoch_{e}.pt``, ``checkpoint_epoch_{e}[_interrupt].pt``, ``training_history.csv``,
    ``calibration_best.json`` -- the file ``serving.calibration_threshold`` reads next to the checkpoint).

    The step is ``TrainStep``'s recipe (zero_grad, forward, criterion, backward, clip 1.0, fused AdamW, dynamic loss
    scaling when a member computes in fp16).  Nothing inside an epoch's loop synchronises with the host: logits,
    labels and the loss go to an ``EpochMetrics`` accumulator on the device, and ``train_epoch`` / ``validate`` read
    one small block back at their end.  Binary classification (2 logits), as the reference's metrics are.

    Deliberate differences from the reference: a bare ``PretrainedBackboneDetector`` (which returns a tuple) is
    accepted the way ``TrainStep`` accepts it (the reference's ``:192`` would hand the tuple to the criterion); no
    ``tqdm`` bars and no sklearn.  Out of scope: gathering metrics across ``DataParallelTrainer`` ranks (each rank
    would see its own shard; the reference has no data parallelism), ``ConfidenceCalibrator`` and
    ``UncertaintyEstimator`` (the reference never calls them), and an epoch loop for ``ImprovedTrainer``
    (``EpochMetrics.compute(average='weighted')`` gives its callers the numbers)."""

    _ALIASES = {"acc": "accuracy", "auc": "auc", "f1score": "f1", "acc_thr": "accuracy_thr", "f1_thr": "f1_thr"}
    _FIELDS = ["Epoch", "Train_Loss", "Train_Acc", "Train_F1", "Val_Loss", "Val_Acc", "Val_F1", "Val_ROC_AUC",
               "Val_Precision", "Val_Recall", "Val_Acc_thr", "Val_Best_thr_acc", "Val_F1_thr", "Val_Best_thr_f1"]

    def __init__(self, model, device="cuda", checkpoint_dir="checkpoints/ensemble", ensemble_method="weighted"):
        self.model = model.to(device)
        self.device = device
        self.checkpoint_dir = Path(checkpoint_dir)
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        self.ensemble_method = ensemble_method
        self.training_history = []
        self.best_metrics = {"epoch": 0, "val_accuracy": 0, "val_auc": 0, "val_f1": 0, "select_metric": "accuracy",
                             "select_score": float("-inf")}
        self.metrics = EpochMetrics(next(self.model.parameters()).device)
        self.loss_scaler = None

    def prepare_optimizers(self, lr: float = 1e-4, weight_decay: float = 1e-5):
        """``optim.AdamW`` + ``clip_grad_norm_(1.0)`` as one fused step, under the reference's scheduler (``:146-154``)"""
        optimizer = FusedAdamW(self.model.parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=1.0)
        fp16 = any(getattr(m, "compute_dtype", None) == "fp16" for m in self.model.modules())
        self.loss_scaler = DynamicLossScaler(optimizer._m.device) if fp16 else None
        optimizer.set_loss_scaler(self.loss_scaler)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0=10, T_mult=2, eta_min=1e-6)
        return optimizer, scheduler

    def _batch(self, batch):
        if isinstance(batch, dict):
            images, labels = batch.get("images", batch.get("frames")), batch["label"]
        else:
            images, labels = batch
        return images.to(self.device, non_blocking=True), labels.to(self.device, non_blocking=True)

    def _logits(self, images):
        out = self.model(images)
        return out[0] if isinstance(out, tuple) else out

    def train_epoch(self, train_loader, optimizer, criterion, epoch):
        """One pass over ``train_loader``; -> loss (mean of the step losses), accuracy, precision, recall, f1, auc."""
        self.model.train()
        self.metrics.reset()
        scaler = getattr(optimizer, "loss_scaler", None)
        for batch in train_loader:
            images, labels = self._batch(batch)
            optimizer.zero_grad(set_to_none=True)
            logits = self._logits(images)
            loss = criterion(logits, labels)
            (scaler.scale(loss) if scaler is not None else loss).backward()
            optimizer.step()
            self.metrics.update(logits.detach(), labels, loss.detach())
        m = self.metrics.compute()  # the pass's one host sync
        return {k: m[k] for k in ("loss", "accuracy", "precision", "recall", "f1", "auc")}

    def validate(self, val_loader, criterion, epoch):
        """-> the metric dict of ``:284-327`` (with ``confusion_matrix`` and, when both classes are present, the
        threshold sweep)."""
        self.model.eval()
        self.metrics.reset()
        with torch.no_grad():
            for batch in val_loader:
                images, labels = self._batch(batch)
                logits = self._logits(images)
                self.metrics.update(logits, labels, criterion(logits, labels))
        return self.metrics.compute()

    def _check_runtimes(self) -> None:
        """the epoch-end ``B0Runtime.check_status`` (a timed-out software barrier of any trunk plan raises); the
        device is idle here, ``validate`` has just read its results back"""
        from .backbone import B0Runtime

        for m in self.model.modules():
            rt = getattr(m, "_runtime", None)
            if isinstance(rt, B0Runtime):
                rt.check_status(synchronize=False)

    def train(self, train_loader, val_loader, epochs: int = 100, lr: float = 1e-4, weight_decay: float = 1e-5,
              start_epoch: int = 1, class_weights=None, select_metric: str = "accuracy"):
        if start_epoch < 1:
            raise ValueError("start_epoch must be >= 1")
        optimizer, scheduler = self.prepare_optimizers(lr=lr, weight_decay=weight_decay)
        if class_weights is None:
            class_weights = self._infer_class_weights(train_loader)
        criterion = WeightedCrossEntropyLoss(weight=torch.as_tensor(class_weights, dtype=torch.float32)).to(self.device)
        logger.info("ensemble training: %d epochs, method %s, device %s, lr %g, weight decay %g", epochs,
                    self.ensemble_method, self.device, lr, weight_decay)
        current_epoch = start_epoch
        try:
            for epoch in range(start_epoch, epochs + 1):
                current_epoch = epoch
                train_metrics = self.train_epoch(train_loader, optimizer, criterion, epoch)
                val_metrics = self.validate(val_loader, criterion, epoch)
                self._check_runtimes()
                scheduler.step()
                self.training_history.append({"epoch": epoch, "train": train_metrics, "val": val_metrics})
                self._save_history()

                key = (select_metric or "accuracy").strip().lower()
                score = None
                if key in val_metrics:
                    score = float(val_metrics[key])
                else:
                    alias = self._ALIASES.get(key)
                    if alias and alias in val_metrics:
                        score = float(val_metrics[alias])
                if score is None:
                    score = float(val_metrics.get("accuracy", 0.0))
                    key = "accuracy"
                best_score = float(self.best_metrics.get("select_score", float("-inf")))
                if str(self.best_metrics.get("select_metric", key)) != key:  # another metric: start over
                    best_score = float("-inf")
                if score > best_score:
                    self.best_metrics = {"epoch": epoch, "val_accuracy": float(val_metrics.get("accuracy", 0.0)),
                                         "val_auc": float(val_metrics.get("auc", 0.0)),
                                         "val_f1": float(val_metrics.get("f1", 0.0)), "select_metric": key,
                                         "select_score": float(score)}
                    self._save_checkpoint(epoch, is_best=True)
                    self._save_calibration(val_metrics)
                    logger.info("epoch %d: new best (%s = %.4f)", epoch, key, score)
                if epoch % 10 == 0:
                    self._save_checkpoint(epoch, is_best=False)
        except KeyboardInterrupt:
            logger.warning("training interrupted: saving checkpoint and history (epoch %s)", current_epoch)
            self._save_checkpoint(current_epoch, is_best=False, tag="interrupt")
            self._save_history()
            return
        self._save_history()

    def _save_calibration(self, val_metrics) -> None:
        """the thresholds of the best epoch, for inference (``:477-483``)"""
        payload = {"epoch": int(self.best_metrics.get("epoch", 0) or 0),
                   "best_thr_accuracy": float(val_metrics.get("best_thr_accuracy", 0.5)),
                   "accuracy_thr": float(val_metrics.get("accuracy_thr", 0.0)),
                   "best_thr_f1": float(val_metrics.get("best_thr_f1", 0.5)),
                   "f1_thr": float(val_metrics.get("f1_thr", 0.0))}
        (self.checkpoint_dir / "calibration_best.json").write_text(json.dumps(payload, indent=2))

    def _infer_class_weights(self, train_loader) -> torch.Tensor:
        """inverse-frequency weights (0 = real, 1 = fake) from the dataset's file names when it has them
        (``Subset(VideoFacesDataset)``), else from one pass over the loader's labels (``:491-546``)"""
        ds = getattr(train_loader, "dataset", None)
        base = getattr(ds, "dataset", ds)
        indices = getattr(ds, "indices", None)
        n_real = n_fake = 0
        if base is not None and hasattr(base, "files") and hasattr(base, "infer_label") and indices is not None:
            try:
                for i in indices:
                    y = int(base.infer_label(getattr(base.files[i], "name", str(base.files[i]))))
                    n_real += y == 0
                    n_fake += y == 1
            except Exception:
                n_real = n_fake = 0
        if n_real + n_fake == 0:
            for batch in train_loader:
                labels = None
                if isinstance(batch, dict):
                    labels = batch.get("label")
                elif isinstance(batch, (tuple, list)) and len(batch) >= 2:
                    labels = batch[1]
                if labels is None:
                    continue
                for y in labels.detach().cpu().numpy().tolist():
                    n_real += int(y) == 0
                    n_fake += int(y) == 1
        total = max(1, n_real + n_fake)
        n_real, n_fake = max(1, n_real), max(1, n_fake)
        return torch.tensor([total / (2.0 * n_real), total / (2.0 * n_fake)], device=self.device, dtype=torch.float32)

    def _save_checkpoint(self, epoch: int, is_best: bool = False, tag=None) -> None:
        if is_best:
            checkpoint.save_state_dict(self.model, self.checkpoint_dir / "checkpoint_best.pt")
            # the best-at-epoch snapshot is written once per epoch number and never overwritten
            epoch_best = self.checkpoint_dir / f"checkpoint_best_epoch_{epoch}.pt"
            if not epoch_best.exists():
                checkpoint.save_state_dict(self.model, epoch_best)
            return
        name = f"checkpoint_epoch_{epoch}_{tag}.pt" if tag else f"checkpoint_epoch_{epoch}.pt"
        checkpoint.save_state_dict(self.model, self.checkpoint_dir / name)

    def _save_history(self) -> None:
        with open(self.checkpoint_dir / "training_history.csv", "w", newline="") as f:
            writer = csv.DictWriter(f, fieldnames=self._FIELDS)
            writer.writeheader()
            for record in self.training_history:
                v = record.get("val", {}) or {}
                writer.writerow({
                    "Epoch": record["epoch"], "Train_Loss": record["train"]["loss"],
                    "Train_Acc": record["train"]["accuracy"], "Train_F1": record["train"]["f1"],
                    "Val_Loss": v.get("loss", 0.0), "Val_Acc": v.get("accuracy", 0.0), "Val_F1": v.get("f1", 0.0),
                    "Val_ROC_AUC": v.get("auc", 0.0), "Val_Precision": v.get("precision", 0.0),
                    "Val_Recall": v.get("recall", 0.0), "Val_Acc_thr": v.get("accuracy_thr", ""),
                    "Val_Best_thr_acc": v.get("best_thr_accuracy", ""), "Val_F1_thr": v.get("f1_thr", ""),
                    "Val_Best_thr_f1": v.get("best_thr_f1", ""),
                })
