"""Numpy restatement of the device augmentation chain (``csrc/k_augment.hip``) and the case grid of its tests.

Every function states one stage with the kernel's operation order, in integers or in fp32 / fp64 numpy scalars
and arrays (one rounding per operation, no fused multiply-add), so the kernel, built without floating-point
contraction, is compared with ``chain`` for exact equality; the stages themselves are held to Pillow's results
in ``tests/golden/augment.npz`` (``tests/golden/make_augment_golden.py``)."""
import zlib

import numpy as np

PI, PF = 12, 6
FLIP, JITTER, GRAY, DOWNUP, BLUR = 1, 2, 4, 8, 16
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- stages
def coeffs(insz, outsz):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc, bilinear, box (0, insz) -> [(xmin, [k...])]"""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    rows = []
    for xx in range(outsz):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), insz)
        w = [max(0.0, 1.0 - abs((x + xmin - c + 0.5) * ss)) for x in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        rows.append((xmin, [int(0.5 + v * 4194304.0) for v in w]))
    return rows


def _pass(a, rows):
    """one pass along axis 1 with a uint8 result"""
    o = np.zeros((a.shape[0], len(rows), a.shape[2]), np.uint8)
    for xx, (xmin, k) in enumerate(rows):
        s = np.full((a.shape[0], a.shape[2]), 1 << 21, np.int64)
        for i, kk in enumerate(k):
            s += a[:, xmin + i, :].astype(np.int64) * kk
        o[:, xx, :] = np.clip(s >> 22, 0, 255)
    return o


def resize(a, oh, ow):
    """``Image.resize((ow, oh), BILINEAR)`` of the whole of ``a``: horizontal pass first, uint8 between"""
    h, w = a.shape[:2]
    if (h, w) == (oh, ow):
        return a.copy()
    t = _pass(a, coeffs(w, ow))
    return _pass(t.transpose(1, 0, 2), coeffs(h, oh)).transpose(1, 0, 2)


def luma(a):
    a = a.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, x, f):
    """``Image.blend(d, x, f)`` on uint8 arrays, fp32"""
    f = f32(f)
    df = d.astype(np.int32).astype(f32)
    t = df + f * (x.astype(np.int32) - d.astype(np.int32)).astype(f32)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness(a, f):
    return blend(np.zeros_like(a), a, f)


def contrast(a, f):
    m = int(int(luma(a).astype(np.int64).sum()) / (a.shape[0] * a.shape[1]) + 0.5)
    return blend(np.full_like(a, m), a, f)


def saturation(a, f):
    return blend(np.repeat(luma(a)[..., None], 3, 2), a, f)


def rgb2hsv(a):
    """Pillow's rgb2hsv_row (Convert.c)"""
    r, g, b = (a[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eq = maxc == minc
    cr = (maxc - minc).astype(f32)
    crs = np.where(eq, f32(1), cr)
    s = cr / np.where(maxc == 0, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / crs for c in (r, g, b))
    h = np.where(r == maxc, (bc - gc).astype(f64),
                 np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64)))
    t = h.astype(f32).astype(f64) / 6.0 + 1.0
    h = (t - np.floor(t)).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(eq, 0, uh), np.where(eq, 0, us), maxc], -1).astype(np.uint8)


def _cround(x):
    r = np.floor(x)
    return (r + ((x - r) >= 0.5)).astype(np.int32)


def hsv2rgb(a):
    """Pillow's hsv2rgb (Convert.c)"""
    s, v = a[..., 1], a[..., 2]
    h6 = a[..., 0].astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i.astype(f32).astype(f64)).astype(f32).astype(f64)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32).astype(f64)
    vf = v.astype(f32).astype(f64)
    p = np.clip(_cround(vf * (1.0 - fs)), 0, 255)
    q = np.clip(_cround(vf * (1.0 - fs * f)), 0, 255)
    t = np.clip(_cround(vf * (1.0 - fs * (1.0 - f))), 0, 255)
    i = i.astype(np.int32) % 6
    vi = v.astype(np.int32)
    rgb = np.stack([np.choose(i, [vi, q, p, p, t, vi]), np.choose(i, [t, vi, vi, q, p, p]),
                    np.choose(i, [p, p, t, vi, vi, q])], -1)
    return np.where((s == 0)[..., None], vi[..., None], rgb).astype(np.uint8)


def hue(a, shift):
    hsv = rgb2hsv(a)
    hsv[..., 0] += np.uint8(shift)
    return hsv2rgb(hsv)


def grayscale(a):
    return np.repeat(luma(a)[..., None], 3, 2)


def blur(a, k):
    """3x3 blur, reflect padding, weights k[dy] * k[dx], summed in row-major order in fp32, round half to even"""
    k = np.asarray(k, f32)
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="reflect").astype(f32)
    h, w = a.shape[:2]
    acc = np.zeros(a.shape, f32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + (k[dy] * k[dx]) * p[dy:dy + h, dx:dx + w]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def chain(a, pi, pf, out_hw, stages=FLIP | JITTER | GRAY | DOWNUP | BLUR):
    """the whole chain on one frame ``a`` (H, W, 3) with its table rows"""
    flags = int(pi[0]) & stages
    i, j, h, w = (int(v) for v in pi[1:5])
    x = resize(a[i:i + h, j:j + w], *out_hw)
    if flags & FLIP:
        x = x[:, ::-1].copy()
    if flags & JITTER:
        for op in pi[5:9]:
            x = (brightness, contrast, saturation)[op](x, pf[op]) if op < 3 else hue(x, int(pi[9]))
    if flags & GRAY:
        x = grayscale(x)
    if flags & DOWNUP:
        x = resize(resize(x, int(pi[10]), int(pi[11])), *out_hw)
    if flags & BLUR:
        x = blur(x, pf[3:6])
    return x


def valid_row(pi, pf, src_hw, out_hw):
    """the C ABI's validation rules (include/dfd_hip.h) on one row"""
    (h, w), (oh, ow) = src_hw, out_hw
    return bool(0 <= pi[0] < 32 and pi[1] >= 0 and pi[2] >= 0 and pi[3] >= 1 and pi[4] >= 1 and pi[1] + pi[3] <= h
                and pi[2] + pi[4] <= w and sorted(int(v) for v in pi[5:9]) == [0, 1, 2, 3] and 0 <= pi[9] <= 255
                and 1 <= pi[10] <= max(oh, 8) and 1 <= pi[11] <= max(ow, 8)
                and not (pi[0] & BLUR and (oh < 2 or ow < 2)) and np.isfinite(pf).all())


# ---------------------------------------------------------------- inputs and the case grid
SOURCES = {"odd": (37, 41, 11), "tiny": (12, 10, 12), "full": (224, 224, 13)}  # name: (H, W, seed)


def source(name):
    """noise on a smooth ramp (so crops, means and blurs all have something to see); RandomState's stream is frozen"""
    h, w, seed = SOURCES[name]
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // (h + w - 2)], -1)
    return np.clip(ramp // 2 + rs.randint(0, 160, (h, w, 3)), 0, 255).astype(np.uint8)


def blur_taps(sigma):
    """torchvision's _get_gaussian_kernel1d(3, sigma) in fp32"""
    import torch

    x = torch.linspace(-1.0, 1.0, 3, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    return (pdf / pdf.sum()).numpy()


def downup_size(out_hw, s):
    return max(8, int(out_hw[0] * s)), max(8, int(out_hw[1] * s))


def row(src_hw, out_hw, box=None, flags=0, perm=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0), hue_f=0.0, s=0.9, sigma=1.0):
    h, w = src_hw
    i, j, bh, bw = box or (0, 0, h, w)
    h2, w2 = downup_size(out_hw, s)
    pi = np.array([flags, i, j, bh, bw, *perm, int(hue_f * 255) % 256, h2, w2], np.int32)
    pf = np.array([*factors, *blur_taps(sigma)], f32)
    return pi, pf


def _boxes(h, w):
    return {"whole": (0, 0, h, w), "corner": (h - h * 3 // 4, w - w * 4 // 5, h * 3 // 4, w * 4 // 5),
            "inset": (1, 1, h - 2, w - 2)}


def cases():
    """-> [(name, source name, out_hw, pi, pf, s or None, sigma or None)]; single-stage cases keep the source size
    and the whole box so that the one stage is all that acts (a jitter case runs its four operations, the others
    at factor 1 / shift 0, as ColorJitter does)."""
    out = []

    def add(name, src, out_hw, s=None, sigma=None, **kw):
        hw = SOURCES[src][:2]
        pi, pf = row(hw, out_hw, **kw, **({"s": s} if s is not None else {}),
                     **({"sigma": sigma} if sigma is not None else {}))
        out.append((name, src, tuple(out_hw), pi, pf, s, sigma))

    for src in ("odd", "tiny"):
        hw = SOURCES[src][:2]
        for oname, ohw in (("24x20", (24, 20)), ("41x37", (41, 37))):
            for bname, box in _boxes(*hw).items():
                add(f"resize/{src}/{oname}/{bname}", src, ohw, box=box)
    add("resize/odd/224x224/whole", "odd", (224, 224))
    for bname, box in _boxes(224, 224).items():
        add(f"resize/full/224x224/{bname}", "full", (224, 224), box=box)
    add("resize/full/41x37/whole", "full", (41, 37))  # support 5.5 / 6.1: 13 and 15 taps
    odd = SOURCES["odd"][:2]
    add("flip/odd", "odd", odd, flags=FLIP)
    add("flip/tiny", "tiny", SOURCES["tiny"][:2], flags=FLIP)
    for k, (lo, hi) in enumerate(((0.75, 1.25), (0.75, 1.25), (0.8, 1.2))):
        for f in (lo, hi):
            fac = [1.0, 1.0, 1.0]
            fac[k] = f
            add(f"{('brightness', 'contrast', 'saturation')[k]}/{f}", "odd", odd, flags=JITTER, factors=tuple(fac))
    for hf in (-0.02, 0.02):
        add(f"hue/{hf}", "odd", odd, flags=JITTER, hue_f=hf)
    for perm in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)):
        add(f"jitter/{''.join(map(str, perm))}", "odd", odd, flags=JITTER, perm=perm, factors=(1.2, 0.8, 1.15),
            hue_f=0.015)
    add("jitter/full", "full", (224, 224), flags=JITTER, perm=(1, 0, 3, 2), factors=(0.8, 1.25, 0.85), hue_f=-0.02)
    add("gray/odd", "odd", odd, flags=GRAY)
    for s in (0.55, 0.9):
        add(f"downup/odd/{s}", "odd", odd, flags=DOWNUP, s=s)
    add("downup/tiny/0.55", "tiny", SOURCES["tiny"][:2], flags=DOWNUP, s=0.55)  # max(8, ...) clamps both sizes
    add("downup/full/0.55", "full", (224, 224), flags=DOWNUP, s=0.55)
    for sg in (0.1, 2.0):
        add(f"blur/odd/{sg}", "odd", odd, flags=BLUR, sigma=sg)
    add("blur/tiny/2.0", "tiny", SOURCES["tiny"][:2], flags=BLUR, sigma=2.0)
    add("blur/full/1.0", "full", (224, 224), flags=BLUR, sigma=1.0)
    return out


ALL = FLIP | JITTER | GRAY | DOWNUP | BLUR


def composed_cases():
    """-> [(name, source name, out_hw, params_i (N, PI), params_f (N, PF))]: whole chains, compared with ``chain``"""
    out = []
    odd, full = SOURCES["odd"][:2], SOURCES["full"][:2]
    a = [row(odd, (24, 20), box=(3, 2, 30, 33)),  # all off
         row(odd, (24, 20), box=(3, 2, 30, 33), flags=ALL, perm=(2, 3, 1, 0), factors=(1.2, 0.8, 1.1), hue_f=0.02,
             s=0.55, sigma=0.7),
         row(odd, (24, 20), box=(7, 8, 30, 33), flags=ALL & ~GRAY, perm=(3, 0, 2, 1), factors=(0.75, 1.25, 0.8),
             hue_f=-0.02, s=0.9, sigma=2.0)]
    out.append(("odd->24x20", "odd", (24, 20), np.stack([r[0] for r in a]), np.stack([r[1] for r in a])))
    b = [row(full, full, box=(20 + 3 * n, 8 * n, 180 + n, 190 - 2 * n), flags=ALL & ~(GRAY if n % 2 else 0),
             perm=((0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 0, 1), (1, 0, 3, 2), (3, 2, 1, 0))[n],
             factors=(0.8 + 0.1 * n, 1.25 - 0.1 * n, 0.85 + 0.07 * n), hue_f=-0.02 + 0.01 * n, s=0.55 + 0.08 * n,
             sigma=0.1 + 0.45 * n) for n in range(5)]
    out.append(("full->224x224 all on", "full", full, np.stack([r[0] for r in b]), np.stack([r[1] for r in b])))
    c = [row(full, (300, 260), box=(0, 0, 224, 224), flags=ALL, perm=(1, 2, 3, 0), factors=(1.1, 0.9, 1.2),
             hue_f=0.01, s=0.6, sigma=1.3), row(full, (300, 260), box=(10, 20, 200, 190))]
    out.append(("full->300x260 (scratch path)", "full", (300, 260), np.stack([r[0] for r in c]),
                np.stack([r[1] for r in c])))
    return out


def digest(a):
    return np.array([zlib.crc32(np.ascontiguousarray(a).tobytes())], np.uint32)


GOLDEN_ROWS = (0, 111, 223)  # what a 224 x 224 case stores next to its checksum
