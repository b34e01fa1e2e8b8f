"""``torch.ops.dfd.*``: the hot-path kernels registered as PyTorch operators.

The drop-in boundary is the ``nn.Module`` contract; under it the modules call these operators, and
under the operators sits the C ABI of ``libdfd_hip.so`` (``include/dfd_hip.h``).  Registration uses
``torch.library.custom_op`` (schema, HIP implementation on the "cuda" device type, a fake/meta
implementation for shape propagation, and autograd where the op is differentiable on its own):

  dfd::b0_trunk_forward / dfd::b0_trunk_backward   the EfficientNet-B0 trunk plan (timm conv_stem ..
                                                   global_pool, src/pretrained_detector.py:116)
  dfd::weighted_cross_entropy (+ _backward)        nn.CrossEntropyLoss(weight) (ensemble_trainer.py:358)
  dfd::classification_loss (+ _backward)           FocalLoss / nn.CrossEntropyLoss(weight, label_smoothing)
                                                   (train_improved.py:29-78, 136-150)
  dfd::metrics_append, dfd::metrics_finalize       the per-step bookkeeping and the per-epoch reductions behind the
                                                   metrics of train_epoch / validate (ensemble_trainer.py:203-211,
                                                   266-329), kept on the device: one host read per epoch
  dfd::ensemble_decide                             serving an EnsembleDetector: the combination of the members'
                                                   outputs (pretrained_detector.py:196-216) and the fp32 values of the
                                                   app's decision step (app.py:2090-2143) for a batch of videos
  dfd::grad_norm, dfd::adam_step                   clip_grad_norm_(1.0) + AdamW (ensemble_trainer.py:196-200)
  dfd::grad_norm_scaled, dfd::adam_step_scaled,    the same under dynamic loss scaling (fp16 training:
  dfd::loss_scale_update                           GradScaler unscale_ / step / update, on the device)
  dfd::collate_frames                              the collate gather + /255 (train.py:38-61)
  dfd::augment_frames                              VideoFacesDataset's train / eval transforms (dataset.py:125-142)
  dfd::augment_frames_jpeg                         the same with the JPEG recompression stage (dataset.py:83-105)

Every operator runs on the caller's current HIP stream and raises ``RuntimeError`` (``DFDError``) on
failure: there is no CPU implementation and no fallback.  The trunk operators take the plan as an
integer handle owned by the module's ``B0Runtime`` (per-model state, no process-wide cache)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib

FEATURE_DIM = 1280
INPUT_F32, INPUT_U8 = 0, 1


def _norm_arr(norm: List[float]):
    import ctypes

    if len(norm) != 6:
        raise _lib.DFDError("input normalisation needs 3 means and 3 stds")
    return (ctypes.c_float * 6)(*[float(v) for v in norm])


def _strides(x: Tensor):
    import ctypes

    return (ctypes.c_int64 * 4)(*x.stride())


# ---------------------------------------------------------------- B0 trunk
@torch.library.custom_op("dfd::b0_trunk_forward", mutates_args=("buffers",), device_types="cuda")
def b0_trunk_forward(frames: Tensor, plan: int, params: Tensor, buffers: Tensor, norm: List[float], training: bool,
                     momentum: float) -> Tuple[Tensor, Tensor]:
    """frames (N,3,H,W) fp32 or uint8, any strides -> (features (N,1280) fp32, saved-activation workspace).
    Train mode updates the BatchNorm running statistics in ``buffers``."""
    lib = _lib.load()
    ws = torch.empty(int(lib.dfd_b0_workspace_bytes(plan)), dtype=torch.uint8, device=frames.device)
    feats = torch.empty(frames.shape[0], FEATURE_DIM, dtype=torch.float32, device=frames.device)
    fmt = INPUT_U8 if frames.dtype == torch.uint8 else INPUT_F32
    _lib.check(lib.dfd_b0_forward_ex(plan, _lib.stream_of(frames.device), frames.data_ptr(), fmt, _strides(frames),
                                     _norm_arr(norm), params.data_ptr(), buffers.data_ptr(), ws.data_ptr(),
                                     feats.data_ptr(), 1 if training else 0, float(momentum)))
    return feats, ws


@b0_trunk_forward.register_fake
def _(frames, plan, params, buffers, norm, training, momentum):
    n = int(_lib.load().dfd_b0_workspace_bytes(plan))
    return frames.new_empty(frames.shape[0], FEATURE_DIM, dtype=torch.float32), frames.new_empty(n, dtype=torch.uint8)


# workspace: the backward reuses its scratch regions (activation gradients, BN/SE partials, slabs)
@torch.library.custom_op("dfd::b0_trunk_backward", mutates_args=("workspace", "grads"), device_types="cuda")
def b0_trunk_backward(frames: Tensor, plan: int, dfeat: Tensor, params: Tensor, workspace: Tensor, grads: Tensor,
                      norm: List[float], training: bool, seg_begin: int, seg_end: int, accumulate: bool) -> None:
    """Backward of trunk segments [seg_begin, seg_end) (output side first) into the flat ``grads``."""
    lib = _lib.load()
    fmt = INPUT_U8 if frames.dtype == torch.uint8 else INPUT_F32
    dfeat = dfeat.contiguous().float()
    _lib.check(lib.dfd_b0_backward_ex(plan, _lib.stream_of(frames.device), frames.data_ptr(), fmt, _strides(frames),
                                      _norm_arr(norm), dfeat.data_ptr(), params.data_ptr(), workspace.data_ptr(),
                                      grads.data_ptr(), 1 if training else 0, int(seg_begin), int(seg_end),
                                      1 if accumulate else 0))


@b0_trunk_backward.register_fake
def _(frames, plan, dfeat, params, workspace, grads, norm, training, seg_begin, seg_end, accumulate):
    return None


# ---------------------------------------------------------------- weighted cross entropy
@torch.library.custom_op("dfd::weighted_cross_entropy", mutates_args=(), device_types="cuda")
def weighted_cross_entropy(logits: Tensor, target: Tensor, weight: Optional[Tensor],
                           ignore_index: int) -> Tuple[Tensor, Tensor]:
    """-> (mean loss (), sum of the applied class weights (1,)), nn.CrossEntropyLoss(weight, reduction='mean')."""
    lib = _lib.load()
    logits = logits.contiguous().float()
    target = target.contiguous().long()
    B, NC = logits.shape
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    _lib.check(lib.dfd_ce_forward(_lib.stream_of(logits.device), logits.data_ptr(), target.data_ptr(),
                                  _lib.ptr(weight), B, NC, ignore_index, out.data_ptr(), out[1:].data_ptr()))
    return out[0].clone(), out[1:].clone()


@weighted_cross_entropy.register_fake
def _(logits, target, weight, ignore_index):
    return logits.new_empty((), dtype=torch.float32), logits.new_empty(1, dtype=torch.float32)


@torch.library.custom_op("dfd::weighted_cross_entropy_backward", mutates_args=(), device_types="cuda")
def weighted_cross_entropy_backward(grad: Tensor, logits: Tensor, target: Tensor, weight: Optional[Tensor],
                                    ignore_index: int, wsum: Tensor) -> Tensor:
    lib = _lib.load()
    logits = logits.contiguous().float()
    target = target.contiguous().long()
    B, NC = logits.shape
    g = grad.contiguous().float().reshape(1)
    d = torch.empty_like(logits)
    _lib.check(lib.dfd_ce_backward(_lib.stream_of(logits.device), logits.data_ptr(), target.data_ptr(),
                                   _lib.ptr(weight), B, NC, ignore_index, wsum.data_ptr(), g.data_ptr(),
                                   d.data_ptr()))
    return d


@weighted_cross_entropy_backward.register_fake
def _(grad, logits, target, weight, ignore_index, wsum):
    return torch.empty_like(logits, dtype=torch.float32)


def _ce_setup(ctx, inputs, output):
    logits, target, weight, ignore_index = inputs
    ctx.save_for_backward(logits, target, output[1])
    ctx.weight, ctx.ignore_index = weight, ignore_index


def _ce_backward(ctx, gloss, _gwsum):
    logits, target, wsum = ctx.saved_tensors
    d = torch.ops.dfd.weighted_cross_entropy_backward(gloss, logits, target, ctx.weight, ctx.ignore_index, wsum)
    return d, None, None, None


weighted_cross_entropy.register_autograd(_ce_backward, setup_context=_ce_setup)


# ---------------------------------------------------------------- focal / label-smoothed losses
LOSS_MODES = {"focal": 0, "ce": 1}
LOSS_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _loss_codes(mode: str, reduction: str):
    if mode not in LOSS_MODES or reduction not in LOSS_REDUCTIONS:
        raise _lib.DFDError(f"classification_loss: unknown mode {mode!r} or reduction {reduction!r}")
    return LOSS_MODES[mode], LOSS_REDUCTIONS[reduction]


def _loss_work_floats(B: int, C: int) -> int:
    n = int(_lib.load().dfd_loss_work_floats(B, C))
    if n < 0:
        raise _lib.DFDError(f"classification_loss: needs B >= 1 and 1 <= C <= 1024 (got B = {B}, C = {C})")
    return n


@torch.library.custom_op("dfd::classification_loss", mutates_args=(), device_types="cuda")
def classification_loss(logits: Tensor, target: Tensor, weight: Optional[Tensor], mode: str, reduction: str,
                        gamma: float, label_smoothing: float, ignore_index: int) -> Tuple[Tensor, Tensor]:
    """mode 'focal': FocalLoss(gamma, weight, label_smoothing); 'ce': cross_entropy(weight, label_smoothing,
    ignore_index).  -> (loss: () for 'mean' / 'sum', (B,) for 'none'; the backward's workspace)."""
    lib = _lib.load()
    m, r = _loss_codes(mode, reduction)
    logits = logits.contiguous().float()
    target = target.contiguous().long()
    weight = None if weight is None else weight.contiguous().float()
    B, C = logits.shape
    work = torch.empty(_loss_work_floats(B, C), dtype=torch.float32, device=logits.device)
    loss = torch.empty((B,) if reduction == "none" else (), dtype=torch.float32, device=logits.device)
    _lib.check(lib.dfd_loss_forward(_lib.stream_of(logits.device), m, r, logits.data_ptr(), target.data_ptr(),
                                    _lib.ptr(weight), B, C, float(gamma), float(label_smoothing), int(ignore_index),
                                    work.data_ptr(), loss.data_ptr()))
    return loss, work


@classification_loss.register_fake
def _(logits, target, weight, mode, reduction, gamma, label_smoothing, ignore_index):
    B, C = logits.shape
    return (logits.new_empty((B,) if reduction == "none" else (), dtype=torch.float32),
            logits.new_empty(_loss_work_floats(B, C), dtype=torch.float32))


@torch.library.custom_op("dfd::classification_loss_backward", mutates_args=(), device_types="cuda")
def classification_loss_backward(grad: Tensor, target: Tensor, weight: Optional[Tensor], work: Tensor,
                                 num_classes: int, mode: str, reduction: str, gamma: float, label_smoothing: float,
                                 ignore_index: int) -> Tensor:
    """grad: the upstream gradient, () or (B,) like the loss; read on the device.  -> dlogits (B, C) fp32."""
    lib = _lib.load()
    m, r = _loss_codes(mode, reduction)
    target = target.contiguous().long()
    weight = None if weight is None else weight.contiguous().float()
    B, C = target.shape[0], int(num_classes)
    if work.numel() != _loss_work_floats(B, C) or grad.numel() != (B if reduction == "none" else 1):
        raise _lib.DFDError("classification_loss_backward: workspace or gradient of another shape")
    g = grad.contiguous().float()
    d = torch.empty(B, C, dtype=torch.float32, device=work.device)
    _lib.check(lib.dfd_loss_backward(_lib.stream_of(work.device), m, r, target.data_ptr(), _lib.ptr(weight), B, C,
                                     float(gamma), float(label_smoothing), int(ignore_index), work.data_ptr(),
                                     g.data_ptr(), d.data_ptr()))
    return d


@classification_loss_backward.register_fake
def _(grad, target, weight, work, num_classes, mode, reduction, gamma, label_smoothing, ignore_index):
    return work.new_empty(target.shape[0], num_classes, dtype=torch.float32)


def _loss_setup(ctx, inputs, output):
    logits, target, weight, *ctx.args = inputs
    ctx.save_for_backward(target, output[1])
    ctx.weight, ctx.num_classes, ctx.dtype = weight, logits.shape[1], logits.dtype


def _loss_backward(ctx, gloss, _gwork):
    target, work = ctx.saved_tensors
    d = torch.ops.dfd.classification_loss_backward(gloss, target, ctx.weight, work, ctx.num_classes, *ctx.args)
    return (d.to(ctx.dtype), None, None, None, None, None, None, None)


classification_loss.register_autograd(_loss_backward, setup_context=_loss_setup)


# ---------------------------------------------------------------- device-side epoch metrics
METRICS_MAX_THRESHOLDS = 32
METRICS_RESULT_WORDS = 72  # include/dfd_hip.h: DFD_METRICS_RESULT_WORDS, layout at dfd_metrics_finalize


# probs / tags / loss_sums: the epoch's state (metrics.EpochMetrics owns it); rows offset .. offset + B - 1 are written
@torch.library.custom_op("dfd::metrics_append", mutates_args=("probs", "tags", "loss_sums"), device_types="cuda")
def metrics_append(logits: Tensor, labels: Tensor, loss: Optional[Tensor], offset: int, probs: Tensor, tags: Tensor,
                   loss_sums: Tensor) -> None:
    """logits (B, 2), labels (B) int64, loss a device scalar or None -> probs[offset + r] = softmax(logits[r])[1],
    tags[offset + r] = label | prediction << 1 | labelled << 2, loss_sums += (loss, loss * B).  No host sync."""
    if logits.dim() != 2 or logits.shape[1] != 2 or labels.shape != logits.shape[:1]:
        raise _lib.DFDError(f"metrics_append: needs (B, 2) logits and (B) labels, got {tuple(logits.shape)} and "
                            f"{tuple(labels.shape)}")
    if (probs.dtype != torch.float32 or tags.dtype != torch.uint8 or loss_sums.dtype != torch.float64
            or tags.numel() != probs.numel() or loss_sums.numel() != 2
            or not (probs.is_contiguous() and tags.is_contiguous() and loss_sums.is_contiguous())):
        raise _lib.DFDError("metrics_append: state must be fp32 probs, uint8 tags of the same length and 2 fp64 sums")
    logits = logits.contiguous().float()
    labels = labels.contiguous().long()
    loss = None if loss is None else loss.reshape(1).float()
    _lib.check(_lib.load().dfd_metrics_append(_lib.stream_of(logits.device), logits.data_ptr(), labels.data_ptr(),
                                              _lib.ptr(loss), logits.shape[0], int(offset), probs.numel(),
                                              probs.data_ptr(), tags.data_ptr(), loss_sums.data_ptr()))


@metrics_append.register_fake
def _(logits, labels, loss, offset, probs, tags, loss_sums):
    return None


@torch.library.custom_op("dfd::metrics_finalize", mutates_args=(), device_types="cuda")
def metrics_finalize(probs: Tensor, tags: Tensor, n: int, thresholds: List[float]) -> Tensor:
    """-> the int64 result block of the first n rows (counts, confusion counts, U2, per-threshold tp / fp; layout in
    include/dfd_hip.h).  thresholds: at most 32 values, rounded to fp32 here.  Enqueues only."""
    import ctypes

    if probs.dtype != torch.float32 or tags.dtype != torch.uint8 or not 0 <= n <= min(probs.numel(), tags.numel()):
        raise _lib.DFDError("metrics_finalize: needs fp32 probs, uint8 tags and 0 <= n <= their length")
    if len(thresholds) > METRICS_MAX_THRESHOLDS:
        raise _lib.DFDError(f"metrics_finalize: at most {METRICS_MAX_THRESHOLDS} thresholds (got {len(thresholds)})")
    thr = (ctypes.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    out = torch.empty(METRICS_RESULT_WORDS, dtype=torch.int64, device=probs.device)
    _lib.check(_lib.load().dfd_metrics_finalize(_lib.stream_of(probs.device), probs.data_ptr(), tags.data_ptr(),
                                                int(n), thr, len(thresholds), out.data_ptr()))
    return out


@metrics_finalize.register_fake
def _(probs, tags, n, thresholds):
    return probs.new_empty(METRICS_RESULT_WORDS, dtype=torch.int64)


# ---------------------------------------------------------------- serving an ensemble
ENSEMBLE_METHODS = {"average": 0, "weighted": 1, "voting": 2}  # include/dfd_hip.h: DFD_ENSEMBLE_*
ENSEMBLE_BLOCK_BASE = 5  # words in front of the 2M per-member probabilities of a decision-block row


@torch.library.custom_op("dfd::ensemble_decide", mutates_args=(), device_types="cuda")
def ensemble_decide(member_logits: Tensor, member_scores: Tensor, weights: Optional[Tensor], method: str, fake_idx: int,
                    temperature: float) -> Tuple[Tensor, Tensor, Tensor]:
    """member logits (M, V, 2), member frame scores (M, V, T), the raw ensemble weights (M) or None -> the ensemble's
    (logits (V, 2), scores (V, T), decision block (V, 5 + 2M)) of EnsembleDetector.forward and the app's decision step,
    in one launch (layout: include/dfd_hip.h, dfd_ensemble_decide).  Eval only: no autograd.  Enqueues only."""
    if method not in ENSEMBLE_METHODS:
        raise _lib.DFDError(f"ensemble_decide: unknown ensemble method {method!r}")
    if member_logits.dim() != 3 or member_scores.dim() != 3 or member_scores.shape[:2] != member_logits.shape[:2]:
        raise _lib.DFDError(f"ensemble_decide: needs (M, V, C) logits and (M, V, T) scores, got "
                            f"{tuple(member_logits.shape)} and {tuple(member_scores.shape)}")
    M, V, C = (int(d) for d in member_logits.shape)
    T = int(member_scores.shape[2])
    if weights is not None and (weights.dim() != 1 or weights.numel() != M):
        raise _lib.DFDError(f"ensemble_decide: needs {M} ensemble weights, got {tuple(weights.shape)}")
    zl = member_logits.detach().contiguous().float()
    zs = member_scores.detach().contiguous().float()
    w = None if weights is None else weights.detach().contiguous().float()
    lib = _lib.load()
    words = int(lib.dfd_ensemble_decide_floats(M))
    if words < 0:
        _lib.check(-1)
    dev = zl.device
    logits = torch.empty((V, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((V, T), dtype=torch.float32, device=dev)
    block = torch.empty((V, words), dtype=torch.float32, device=dev)
    _lib.check(lib.dfd_ensemble_decide(_lib.stream_of(dev), zl.data_ptr(), zs.data_ptr(), _lib.ptr(w), M, V, C, T,
                                       ENSEMBLE_METHODS[method], int(fake_idx), float(temperature),
                                       logits.data_ptr(), scores.data_ptr(), block.data_ptr()))
    return logits, scores, block


@ensemble_decide.register_fake
def _(member_logits, member_scores, weights, method, fake_idx, temperature):
    M, V = member_logits.shape[0], member_logits.shape[1]
    f32 = torch.float32
    return (member_logits.new_empty((V, 2), dtype=f32), member_logits.new_empty((V, member_scores.shape[2]), dtype=f32),
            member_logits.new_empty((V, ENSEMBLE_BLOCK_BASE + 2 * M), dtype=f32))


# ---------------------------------------------------------------- optimizer
# scratch: the kernel's fixed-order partial sums (written); out: [norm, clip coefficient]
@torch.library.custom_op("dfd::grad_norm", mutates_args=("scratch", "out"), device_types="cuda")
def grad_norm(grads: Tensor, max_norm: float, scratch: Tensor, out: Tensor) -> None:
    """out[0] = ||grads||_2 (fp64 accumulation, fixed order), out[1] = clip coefficient
    min(1, max_norm / (norm + 1e-6)) -- clip_grad_norm_ (torch/nn/utils/clip_grad.py)."""
    _lib.check(_lib.load().dfd_grad_norm(_lib.stream_of(grads.device), grads.data_ptr(), grads.numel(),
                                         float(max_norm), scratch.data_ptr(), out.data_ptr()))


@grad_norm.register_fake
def _(grads, max_norm, scratch, out):
    return None


# grads: with `clip` the kernel writes the clipped gradient back (FusedAdam leaves it in .grad, as
# clip_grad_norm_ does in place)
@torch.library.custom_op("dfd::adam_step", mutates_args=("params", "grads", "exp_avg", "exp_avg_sq"),
                         device_types="cuda")
def adam_step(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
              beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float, decoupled: bool,
              clip: Optional[Tensor]) -> None:
    """One Adam (decoupled=False) / AdamW step over a flat fp32 range, with the clip coefficient of
    dfd::grad_norm applied to the gradient first (torch/optim/adamw.py semantics)."""
    _lib.check(_lib.load().dfd_adam_step(_lib.stream_of(params.device), params.data_ptr(), grads.data_ptr(),
                                         exp_avg.data_ptr(), exp_avg_sq.data_ptr(), params.numel(), float(lr),
                                         float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                         float(grad_scale), 1 if decoupled else 0,
                                         None if clip is None else clip.data_ptr()))


@adam_step.register_fake
def _(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale, decoupled, clip):
    return None


# dynamic loss scaling (fp16 training): `scaler` is the 4-float device state of optim.DynamicLossScaler
@torch.library.custom_op("dfd::grad_norm_scaled", mutates_args=("scaler", "scratch", "out"), device_types="cuda")
def grad_norm_scaled(grads: Tensor, max_norm: float, scaler: Tensor, scratch: Tensor, out: Tensor) -> None:
    """dfd::grad_norm of the SCALED gradient: out[0] = the unscaled norm, scaler[2] = found_inf."""
    _lib.check(_lib.load().dfd_grad_norm_scaled(_lib.stream_of(grads.device), grads.data_ptr(), grads.numel(),
                                                float(max_norm), scaler.data_ptr(), scratch.data_ptr(),
                                                out.data_ptr()))


@grad_norm_scaled.register_fake
def _(grads, max_norm, scaler, scratch, out):
    return None


@torch.library.custom_op("dfd::adam_step_scaled", mutates_args=("params", "grads", "exp_avg", "exp_avg_sq"),
                         device_types="cuda")
def adam_step_scaled(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
                     beta2: float, eps: float, weight_decay: float, grad_scale: float, decoupled: bool,
                     clip: Optional[Tensor], scaler: Tensor) -> None:
    """dfd::adam_step on grads / scale, skipped on device when the scaler saw a non-finite norm; the
    bias corrections count applied steps only (scaler[3])."""
    _lib.check(_lib.load().dfd_adam_step_scaled(_lib.stream_of(params.device), params.data_ptr(), grads.data_ptr(),
                                                exp_avg.data_ptr(), exp_avg_sq.data_ptr(), params.numel(), float(lr),
                                                float(beta1), float(beta2), float(eps), float(weight_decay),
                                                float(grad_scale), 1 if decoupled else 0,
                                                None if clip is None else clip.data_ptr(), scaler.data_ptr()))


@adam_step_scaled.register_fake
def _(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, decoupled, clip, scaler):
    return None


@torch.library.custom_op("dfd::loss_scale_update", mutates_args=("scaler",), device_types="cuda")
def loss_scale_update(scaler: Tensor, growth_factor: float, backoff_factor: float, growth_interval: int) -> None:
    """GradScaler.update on the device state (no host synchronisation)."""
    _lib.check(_lib.load().dfd_loss_scale_update(_lib.stream_of(scaler.device), scaler.data_ptr(),
                                                 float(growth_factor), float(backoff_factor), int(growth_interval)))


@loss_scale_update.register_fake
def _(scaler, growth_factor, backoff_factor, growth_interval):
    return None


# ---------------------------------------------------------------- input pipeline
@torch.library.custom_op("dfd::collate_frames", mutates_args=(), device_types="cuda")
def collate_frames(src: Tensor, sel: Tensor, frame_shape: List[int], to_float: bool) -> Tensor:
    """out[s] = src[sel[s]] (sel < 0: a zero frame), uint8 or fp32 v/255; src (F, *frame_shape) uint8."""
    n = sel.numel()
    fb = 1
    for d in frame_shape:
        fb *= int(d)
    out = torch.empty((n, *frame_shape), dtype=torch.float32 if to_float else torch.uint8, device=src.device)
    _lib.check(_lib.load().dfd_collate_frames(_lib.stream_of(src.device), src.data_ptr(), sel.data_ptr(), n, fb,
                                              1 if to_float else 0, out.data_ptr()))
    return out


@collate_frames.register_fake
def _(src, sel, frame_shape, to_float):
    return src.new_empty((sel.numel(), *frame_shape), dtype=torch.float32 if to_float else torch.uint8)


# ---------------------------------------------------------------- augmentation / eval resize
AUG_PI, AUG_PF = 12, 6  # columns of the two parameter tables (include/dfd_hip.h: DFD_AUG_PI / DFD_AUG_PF)


def _augment_check(src: Tensor, params_i: Tensor, params_f: Tensor, out_size: List[int]) -> Tuple[int, int, int, int, int]:
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
        raise _lib.DFDError(f"augment_frames: frames must be uint8 (N, H, W, 3), got {src.dtype} {tuple(src.shape)}")
    n, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    if len(out_size) != 2:
        raise _lib.DFDError("augment_frames: out_size is (height, width)")
    if (params_i.dtype != torch.int32 or tuple(params_i.shape) != (n, AUG_PI) or params_f.dtype != torch.float32
            or tuple(params_f.shape) != (n, AUG_PF)):
        raise _lib.DFDError(f"augment_frames: parameter tables must be int32 ({n}, {AUG_PI}) and float32 "
                            f"({n}, {AUG_PF}), got {params_i.dtype} {tuple(params_i.shape)} and {params_f.dtype} "
                            f"{tuple(params_f.shape)}")
    return n, h, w, int(out_size[0]), int(out_size[1])


@torch.library.custom_op("dfd::augment_frames", mutates_args=(), device_types="cuda")
def augment_frames(src: Tensor, params_i: Tensor, params_f: Tensor, out_size: List[int]) -> Tensor:
    """src uint8 (N,H,W,3), contiguous, on the device; the parameter tables of ``augment.draw_augment_params``
    (host tensors; device tensors are copied back first) -> uint8 (N, out_h, out_w, 3)."""
    lib = _lib.load()
    n, h, w, oh, ow = _augment_check(src, params_i, params_f, out_size)
    if not src.is_contiguous():
        raise _lib.DFDError("augment_frames: frames must be contiguous NHWC")
    pi, pf = params_i.cpu().contiguous(), params_f.cpu().contiguous()
    nbytes = int(lib.dfd_augment_scratch_bytes(n, h, w, oh, ow))
    if nbytes < 0:
        _lib.check(-1)
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src.device)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=src.device)
    _lib.check(lib.dfd_augment_frames(_lib.stream_of(src.device), src.data_ptr(), n, h, w, pi.data_ptr(),
                                      pf.data_ptr(), oh, ow, out.data_ptr(), scratch.data_ptr(), nbytes))
    return out


@augment_frames.register_fake
def _(src, params_i, params_f, out_size):
    return src.new_empty((src.shape[0], out_size[0], out_size[1], 3), dtype=torch.uint8)


@torch.library.custom_op("dfd::augment_frames_jpeg", mutates_args=(), device_types="cuda")
def augment_frames_jpeg(src: Tensor, params_i: Tensor, params_f: Tensor, quality: Tensor, out_size: List[int]) -> Tensor:
    """``augment_frames`` with the JPEG recompression between the downscale/upscale and the blur, in the same launch.
    quality: int32 (N,) host tensor of ``augment.draw_jpeg_quality``, 0 (stage off for that frame) or 1..100."""
    lib = _lib.load()
    n, h, w, oh, ow = _augment_check(src, params_i, params_f, out_size)
    if quality.dtype != torch.int32 or tuple(quality.shape) != (n,) or quality.device.type != "cpu":
        raise _lib.DFDError(f"augment_frames: quality must be an int32 ({n},) CPU tensor, got {quality.dtype} "
                            f"{tuple(quality.shape)} on {quality.device}")
    if not src.is_contiguous():
        raise _lib.DFDError("augment_frames: frames must be contiguous NHWC")
    pi, pf, q = params_i.cpu().contiguous(), params_f.cpu().contiguous(), quality.contiguous()
    nbytes = int(lib.dfd_augment_jpeg_scratch_bytes(n, h, w, oh, ow))
    if nbytes < 0:
        _lib.check(-1)
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=src.device)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=src.device)
    _lib.check(lib.dfd_augment_frames_jpeg(_lib.stream_of(src.device), src.data_ptr(), n, h, w, pi.data_ptr(),
                                           pf.data_ptr(), q.data_ptr(), oh, ow, out.data_ptr(), scratch.data_ptr(),
                                           nbytes))
    return out


@augment_frames_jpeg.register_fake
def _(src, params_i, params_f, quality, out_size):
    return src.new_empty((src.shape[0], out_size[0], out_size[1], 3), dtype=torch.uint8)


OPS = ("b0_trunk_forward", "b0_trunk_backward", "weighted_cross_entropy", "weighted_cross_entropy_backward",
       "grad_norm", "adam_step", "grad_norm_scaled", "adam_step_scaled", "loss_scale_update", "collate_frames")
# the losses of the ViT+GCN trainer (losses.FocalLoss / SmoothedCrossEntropyLoss)
LOSS_OPS = ("classification_loss", "classification_loss_backward")
# the epoch accumulator of metrics.EpochMetrics / trainer.EnsembleTrainer
METRICS_OPS = ("metrics_append", "metrics_finalize")
# the train / eval transforms in front of the models (augment.TrainAugment / resize_frames)
AUGMENT_OPS = ("augment_frames", "augment_frames_jpeg")
# the ensemble combination and decision block of serving.FrameClassifierService
SERVING_OPS = ("ensemble_decide",)
