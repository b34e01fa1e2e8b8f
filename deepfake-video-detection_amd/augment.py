"""Train-time augmentation and the eval resize of the face crops, on the device.

The reference trains every model behind ``VideoFacesDataset(augment=True)`` (``src/dataset.py:131-142``):
per frame, on Pillow images on the host, ``RandomResizedCrop(scale 0.75-1, ratio 0.9-1.1)``, a horizontal
flip, ``ColorJitter(0.25, 0.25, 0.2, 0.02)`` (p 0.7), ``RandomGrayscale(0.05)``, a bilinear
downscale/upscale (p 0.25), a JPEG recompression (p 0.5) and ``GaussianBlur(3)`` (p 0.25); its eval
transform is ``T.Resize(image_size)``.  Here the random draws stay on the host (a row of integers and
floats per frame, ``draw_augment_params``) and the byte work runs in one HIP launch on the uint8 crops
that ``pipeline.collate_clips(out="uint8")`` already keeps on the device
(``torch.ops.dfd.augment_frames`` -> ``dfd_augment_frames``, ``csrc/k_augment.hip``).  Every stage
restates Pillow's arithmetic (the backend torchvision documents for PIL inputs) and is held to Pillow's
results by ``tests/test_augment_*.py``.

The JPEG recompression (``_RandomJPEGCompression``: ``save(format='JPEG', quality=q, optimize=True)`` and
``open().convert('RGB')``, p 0.5, q 35-95) is a stage of the same launch, between the downscale/upscale and the
blur (``torch.ops.dfd.augment_frames_jpeg`` -> ``dfd_augment_frames_jpeg``): libjpeg-turbo's baseline 4:2:0 round
trip restated in 32-bit integers, byte for byte what Pillow returns (``tests/golden/augment_jpeg.npz``).  Its
quality travels beside the tables as an int32 ``(N,)`` array (0: stage off for that frame), drawn by
``draw_jpeg_quality``.  It is opt-in, ``TrainAugment(..., jpeg=True)``: the default chain and the draws of
``draw_augment_params`` are what they were before the stage existed.

Parameter tables (``include/dfd_hip.h``), one row per frame:

  ``params_i`` int32 (N, 12): flags (``FLIP | JITTER | GRAY | DOWNUP | BLUR``), crop box ``i, j, h, w``
  (top, left, height, width), the four jitter operations in application order (0 brightness, 1 contrast,
  2 saturation, 3 hue), the hue shift ``int(hue * 255) mod 256``, and ``h2, w2`` of the downscale/upscale;
  ``params_f`` float32 (N, 6): brightness, contrast, saturation factors and the three blur taps.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops  # noqa: F401  (registers torch.ops.dfd.*)
from .ops import AUG_PF, AUG_PI

FLIP, JITTER, GRAY, DOWNUP, BLUR = 1, 2, 4, 8, 16
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
_DRAWS = 37  # uniforms per frame


def blur_taps(sigma) -> np.ndarray:
    """torchvision's ``_get_gaussian_kernel1d(3, sigma)`` in fp32: exp(-0.5 (x / sigma)^2) at x = -1, 0, 1,
    normalised.  sigma: scalar or (N,) -> (..., 3) float32."""
    s = torch.as_tensor(np.asarray(sigma, dtype=np.float32)).reshape(-1, 1)
    x = torch.linspace(-1.0, 1.0, 3, dtype=torch.float32).reshape(1, 3)
    pdf = torch.exp(-0.5 * (x / s).pow(2))
    k = (pdf / pdf.sum(dim=1, keepdim=True)).numpy()
    return k.reshape(np.shape(sigma) + (3,))


def identity_params(n: int, src_hw, out_hw=None):
    """Tables with every stage off and the full-frame box: the eval transform ``T.Resize(out_hw)``."""
    h, w = int(src_hw[0]), int(src_hw[1])
    oh, ow = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    pi = np.zeros((n, AUG_PI), dtype=np.int32)
    pi[:, 1:5] = (0, 0, h, w)
    pi[:, 5:9] = (0, 1, 2, 3)
    pi[:, 10:12] = (oh, ow)
    pf = np.zeros((n, AUG_PF), dtype=np.float32)
    pf[:, 0:3] = 1.0
    pf[:, 3:6] = (0.0, 1.0, 0.0)
    return torch.from_numpy(pi), torch.from_numpy(pf)


def draw_augment_params(n: int, src_hw, out_hw, generator: torch.Generator | None = None, *,
                        scale=(0.75, 1.0), ratio=(0.9, 1.1), flip_p=0.5, jitter_p=0.7, brightness=0.25,
                        contrast=0.25, saturation=0.2, hue=0.02, gray_p=0.05, downup_p=0.25,
                        downup_scale=(0.55, 0.9), blur_p=0.25, blur_sigma=(0.1, 2.0)):
    """Draw the parameter tables of ``n`` frames of ``src_hw`` augmented to ``out_hw`` -> ``(params_i,
    params_f)`` as CPU tensors.  The defaults are the reference's numbers (``dataset.py:135-141``); one
    independent draw per frame, as the reference transforms each face on its own.

    The DISTRIBUTIONS follow the reference's transforms: ``RandomResizedCrop.get_params`` (10 tries of
    area x log-uniform ratio, then the centre-crop fallback), ``ColorJitter.get_params`` (a random order of
    the four operations, factors uniform in ``[max(0, 1 - v), 1 + v]``, hue uniform in ``[-hue, hue]``),
    ``_RandomDownscaleUpscale`` (``max(8, int(dim * s))``) and ``GaussianBlur`` (sigma uniform).  The
    STREAM of draws is this project's own (37 uniforms per frame from ``generator``): a seed does not
    reproduce what torchvision and ``random`` would have drawn from theirs.  Nothing is drawn here for the JPEG
    recompression: ``draw_jpeg_quality`` draws for it, from the same generator, after this function."""
    h, w = int(src_hw[0]), int(src_hw[1])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    u = torch.rand(n, _DRAWS, dtype=torch.float64, generator=generator).numpy()

    def uni(col, lo, hi):
        return lo + (hi - lo) * col

    # RandomResizedCrop.get_params
    area = h * w * uni(u[:, 0:10], scale[0], scale[1])
    ar = np.exp(uni(u[:, 10:20], math.log(ratio[0]), math.log(ratio[1])))
    cw = np.rint(np.sqrt(area * ar)).astype(np.int64)
    ch = np.rint(np.sqrt(area / ar)).astype(np.int64)
    ok = (cw > 0) & (cw <= w) & (ch > 0) & (ch <= h)
    first = np.argmax(ok, axis=1)
    hit = ok.any(axis=1)
    rows = np.arange(n)
    bh, bw = ch[rows, first], cw[rows, first]
    bi = np.minimum((u[:, 20] * (h - bh + 1)).astype(np.int64), h - bh)
    bj = np.minimum((u[:, 21] * (w - bw + 1)).astype(np.int64), w - bw)
    in_ratio = w / h
    if in_ratio < min(ratio):
        fw, fh = w, int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        fh, fw = h, int(round(h * max(ratio)))
    else:
        fw, fh = w, h
    bh, bw = np.where(hit, bh, fh), np.where(hit, bw, fw)
    bi, bj = np.where(hit, bi, (h - fh) // 2), np.where(hit, bj, (w - fw) // 2)

    flags = (FLIP * (u[:, 22] < flip_p) + JITTER * (u[:, 23] < jitter_p) + GRAY * (u[:, 32] < gray_p)
             + DOWNUP * (u[:, 33] < downup_p) + BLUR * ((u[:, 35] < blur_p) & (oh >= 2) & (ow >= 2)))
    s = uni(u[:, 34], downup_scale[0], downup_scale[1])
    h2 = np.maximum(8, (oh * s).astype(np.int64))
    w2 = np.maximum(8, (ow * s).astype(np.int64))
    hue_f = uni(u[:, 31], -hue, hue)

    pi = np.zeros((n, AUG_PI), dtype=np.int32)
    pi[:, 0] = flags
    pi[:, 1], pi[:, 2], pi[:, 3], pi[:, 4] = bi, bj, bh, bw
    pi[:, 5:9] = np.argsort(u[:, 24:28], axis=1)
    pi[:, 9] = np.trunc(hue_f * 255).astype(np.int64) % 256
    pi[:, 10], pi[:, 11] = h2, w2
    pf = np.zeros((n, AUG_PF), dtype=np.float32)
    pf[:, 0] = uni(u[:, 28], max(0.0, 1 - brightness), 1 + brightness)
    pf[:, 1] = uni(u[:, 29], max(0.0, 1 - contrast), 1 + contrast)
    pf[:, 2] = uni(u[:, 30], max(0.0, 1 - saturation), 1 + saturation)
    pf[:, 3:6] = blur_taps(uni(u[:, 36], blur_sigma[0], blur_sigma[1]).astype(np.float32))
    return torch.from_numpy(pi), torch.from_numpy(pf)


def draw_jpeg_quality(n: int, generator: torch.Generator | None = None, p=0.5, quality=(35, 95)) -> torch.Tensor:
    """Draw the JPEG quality of ``n`` frames -> int32 ``(N,)`` CPU tensor: 0 (the frame skips the stage) or the
    quality.  ``_RandomJPEGCompression`` (``dataset.py:83-105``): applied when ``u0 < p`` (the reference skips on
    ``random.random() > p``), at ``random.randint(lo, hi)``, both ends inclusive.  Two uniforms per frame from
    ``generator``, the project's own stream as in ``draw_augment_params``."""
    lo, hi = int(quality[0]), int(quality[1])
    u = torch.rand(n, 2, dtype=torch.float64, generator=generator).numpy()
    q = np.minimum(lo + np.floor(u[:, 1] * (hi - lo + 1)).astype(np.int64), hi)
    return torch.from_numpy(np.where(u[:, 0] < p, q, 0).astype(np.int32))


def augment_frames(frames: torch.Tensor, params_i: torch.Tensor, params_f: torch.Tensor, out_size,
                   quality: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 (N,H,W,3) on the device + the two tables -> uint8 (N, out_h, out_w, 3); one HIP launch.  With
    ``quality`` (int32 ``(N,)`` CPU tensor, 0 or 1..100 per frame) the launch includes the JPEG recompression."""
    _lib.require_hip(frames, "frames")
    size = [int(out_size[0]), int(out_size[1])]
    if quality is None:
        return torch.ops.dfd.augment_frames(frames, params_i, params_f, size)
    return torch.ops.dfd.augment_frames_jpeg(frames, params_i, params_f, quality, size)


def resize_frames(frames: torch.Tensor, out_size) -> torch.Tensor:
    """The eval transform ``T.Resize(image_size)`` (``dataset.py:125-129``): Pillow's bilinear resize of
    the whole frame."""
    pi, pf = identity_params(int(frames.shape[0]), frames.shape[1:3], out_size)
    return augment_frames(frames, pi, pf, out_size)


class TrainAugment:
    """The train transform on a ``(B,T,3,H,W)`` uint8 batch as ``collate_clips(out="uint8")`` returns it:
    views the batch back to NHWC, draws one row per frame, launches, and returns ``(B,T,3,h,w)`` uint8 in
    the same channels-last layout.

    The JPEG recompression is opt-in: with ``jpeg=True`` a quality per frame is drawn (``draw_jpeg_quality`` with
    ``jpeg_p``, ``jpeg_quality``) after the tables, on the same generator, and the stage runs in the same launch.
    The reference's full train recipe is ``TrainAugment(image_size, generator, jpeg=True)``; the default leaves
    the stage out and draws exactly what it drew before the stage existed."""

    def __init__(self, image_size=(224, 224), generator: torch.Generator | None = None, *, jpeg=False, jpeg_p=0.5,
                 jpeg_quality=(35, 95), **draw_kwargs):
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.generator = generator
        self.jpeg, self.jpeg_p, self.jpeg_quality = bool(jpeg), float(jpeg_p), (int(jpeg_quality[0]), int(jpeg_quality[1]))
        self.draw_kwargs = draw_kwargs

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 5 or x.shape[2] != 3 or x.dtype != torch.uint8:
            raise _lib.DFDError(f"TrainAugment: expected a uint8 (B,T,3,H,W) batch, got {x.dtype} {tuple(x.shape)}")
        b, t, _, h, w = x.shape
        frames = x.permute(0, 1, 3, 4, 2).contiguous().view(b * t, h, w, 3)  # no copy for collate_clips' layout
        pi, pf = draw_augment_params(b * t, (h, w), self.image_size, self.generator, **self.draw_kwargs)
        q = draw_jpeg_quality(b * t, self.generator, self.jpeg_p, self.jpeg_quality) if self.jpeg else None
        out = augment_frames(frames, pi, pf, self.image_size, q)
        return out.view(b, t, *self.image_size, 3).permute(0, 1, 4, 2, 3)
