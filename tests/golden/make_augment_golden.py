"""Golden fixture of the device augmentation chain: ``augment.npz``.

Pillow's results for the single-stage grid of ``tests/augment_helpers.py`` (``cases()``): each case runs the
stages its table row switches on through Pillow the way torchvision's PIL backend does --
``crop().resize(BILINEAR)``, ``transpose(FLIP_LEFT_RIGHT)``, ``ImageEnhance`` brightness / contrast / colour and
the HSV hue shift of ``adjust_hue`` in the row's order, ``convert('L')`` -- the downscale/upscale through the
REFERENCE's own ``VideoFacesDataset._RandomDownscaleUpscale`` (``src/dataset.py:107-123``, imported from a
checkout of the reference under a stub ``torchvision.transforms``; development machine only) with ``random``
patched to the case's scale, and the blur through ``torch.nn.functional.conv2d`` on the CPU (2-D kernel, reflect
padding, ``round``).  Small cases store the whole result; 224 x 224 results store a CRC-32 and three rows.  The
small sources are stored too; the 224 x 224 one is regenerated from its seed.  Also recorded: the largest
difference of the numpy hue restatement against Pillow over all 2^24 colours, and Pillow's version.

    python tests/golden/make_augment_golden.py /path/to/reference
"""
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import PIL  # noqa: E402
import torch  # noqa: E402
from PIL import Image, ImageEnhance  # noqa: E402

import augment_helpers as ah  # noqa: E402


def pil_hue(img, shift):
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def conv_blur(a, k):
    k = torch.from_numpy(np.asarray(k, np.float32))
    k2 = torch.mm(k[:, None], k[None, :]).expand(3, 1, 3, 3)
    x = torch.from_numpy(a).permute(2, 0, 1)[None].float()
    x = torch.nn.functional.pad(x, (1, 1, 1, 1), mode="reflect")
    y = torch.round(torch.nn.functional.conv2d(x, k2, groups=3)).clamp(0, 255).to(torch.uint8)
    return y[0].permute(1, 2, 0).numpy()


def pil_chain(a, pi, pf, out_hw, s, downup):
    flags = int(pi[0])
    i, j, h, w = (int(v) for v in pi[1:5])
    img = Image.fromarray(a).convert("RGB").crop((j, i, j + w, i + h)).resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    if flags & ah.FLIP:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if flags & ah.JITTER:
        for op in pi[5:9]:
            if op == 3:
                img = pil_hue(img, int(pi[9]))
            else:
                enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
                img = enh(img).enhance(float(pf[op]))
    if flags & ah.GRAY:
        g = np.array(img.convert("L"))
        img = Image.fromarray(np.dstack([g, g, g]), "RGB")
    if flags & ah.DOWNUP:
        random.random = lambda: 0.0
        random.uniform = lambda lo, hi: s
        img = downup(p=1.0, min_scale=0.55, max_scale=0.9)(img)
    x = np.array(img)
    if flags & ah.BLUR:
        x = conv_blur(x, pf[3:6])
    return x


def main():
    ref = sys.argv[1]
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, os.path.join(ref, "src"))
    from dataset import VideoFacesDataset  # noqa: E402

    out = {"pillow_version": np.array(PIL.__version__)}
    srcs = {name: ah.source(name) for name in ah.SOURCES}
    for name in ("odd", "tiny"):
        out[f"src/{name}"] = srcs[name]
    for name, src, out_hw, pi, pf, s, sigma in ah.cases():
        want = pil_chain(srcs[src], pi, pf, out_hw, s, VideoFacesDataset._RandomDownscaleUpscale)
        assert want.shape == (*out_hw, 3) and want.dtype == np.uint8
        if pi[0] & ah.DOWNUP:  # the table's (h2, w2) is what the reference computed from s
            assert tuple(pi[10:12]) == (max(8, int(out_hw[0] * s)), max(8, int(out_hw[1] * s)))
        if out_hw == (224, 224):
            out[f"crc/{name}"] = ah.digest(want)
            out[f"rows/{name}"] = want[list(ah.GOLDEN_ROWS)]
        else:
            out[f"out/{name}"] = want
    # hue: the restated HSV conversions against Pillow's over every colour
    n = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(n >> 16) & 255, (n >> 8) & 255, n & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    d1 = np.abs(np.array(Image.fromarray(cube).convert("HSV")).astype(int) - ah.rgb2hsv(cube)).max()
    d2 = np.abs(np.array(Image.fromarray(cube, "HSV").convert("RGB")).astype(int) - ah.hsv2rgb(cube)).max()
    out["hsv_max_diff"] = np.array([d1, d2], np.int64)
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; hsv max diff", d1, d2, "Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
