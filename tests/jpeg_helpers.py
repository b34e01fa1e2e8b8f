"""Numpy restatement of the JPEG recompression stage of the device augmentation chain (``csrc/k_augment.hip``)
and the case grid of its tests.

``jpeg_roundtrip(a, q)`` restates ``img.save(buf, 'JPEG', quality=q, optimize=True)`` followed by
``Image.open(buf).convert('RGB')`` as Pillow's libjpeg-turbo runs it (baseline, 4:2:0, Annex-K tables, islow DCTs,
fancy upsampling): entropy coding is lossless, so the round trip is a function of the pixels and ``q`` made of
32-bit integer stages only.  It is held to Pillow's bytes in ``tests/golden/augment_jpeg.npz``
(``tests/golden/make_jpeg_golden.py``) and the kernel is compared with it for exact equality."""
import zlib

import numpy as np

i32 = np.int32

# Annex K, natural order
LUMINANCE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMINANCE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# jfdctint / jidctint, CONST_BITS 13
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def fix(x):
    return int(x * 65536 + 0.5)


def quant_table(base, q):
    """jpeg_set_quality + jpeg_add_quant_table with force_baseline -> (8, 8) int32"""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.array(base, i32) * s + 50) // 100, 1, 255).reshape(8, 8)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd_part(t0, t1, t2, t3):
    """the shared odd half of both DCTs: (t0, t1, t2, t3) -> the four rotated sums"""
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    return t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4


def _fdct_pass(d, first):
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    o7, o5, o3, o1 = _odd_part(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = (_descale(v, n) for v in (o7, o5, o3, o1))
    return np.stack(o, -1)


def fdct(b):
    """jfdctint on (..., 8, 8) blocks (rows, columns): rows first; the result is scaled by 8"""
    return np.swapaxes(_fdct_pass(np.swapaxes(_fdct_pass(b, True), -1, -2), False), -1, -2)


def _idct_pass(c, first):
    i0, i1, i2, i3, i4, i5, i6, i7 = (c[..., k] for k in range(8))
    z1 = (i2 + i6) * F_0_541
    t2, t3 = z1 - i6 * F_1_847, z1 + i2 * F_0_765
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _odd_part(i7, i5, i3, i1)
    n = 11 if first else 18
    return np.stack([_descale(v, n) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2,
                                              t10 - t3)], -1)


def idct(c):
    """jidctint on (..., 8, 8) dequantised blocks: columns first, then rows and the range-limit table"""
    w = np.swapaxes(_idct_pass(np.swapaxes(c, -1, -2), True), -1, -2)
    x = _idct_pass(w, False) & 1023
    return np.where(x < 128, x + 128, np.where(x < 512, 255, np.where(x < 896, 0, x - 896)))


def _code_plane(p, t):
    """a plane whose sides are multiples of 8 through DCT, quantiser ``t``, dequantiser and inverse DCT"""
    h, w = p.shape
    b = p.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2) - 128
    c = fdct(b)
    d = t * 8
    m = (np.abs(c) + (d >> 1)) // d
    c = np.where(c < 0, -m, m)
    return idct(c * t).swapaxes(1, 2).reshape(h, w)


def _pad(p, mh, mw):
    h, w = p.shape
    return np.pad(p, ((0, -h % mh), (0, -w % mw)), mode="edge")


def jpeg_roundtrip(a, q):
    """uint8 (H, W, 3) RGB through JPEG at quality ``q`` (1..100) and back; ``q`` 0 returns a copy"""
    q = int(q)
    if q == 0:
        return a.copy()
    r, g, b = (a[..., k].astype(i32) for k in range(3))
    h, w = r.shape
    half, off = 1 << 15, 128 << 16
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + half) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + off + half - 1) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + off + half - 1) >> 16
    yd = _code_plane(_pad(y, 8, 8), quant_table(LUMINANCE, q))[:h, :w]
    tc = quant_table(CHROMINANCE, q)
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    dec = []
    for c in (cb, cr):
        c = _pad(c, 2, 16)  # full-resolution columns to a multiple of 16 BEFORE the downsampling
        bias = np.where(np.arange(c.shape[1] // 2) % 2 == 0, 1, 2)[None, :].astype(i32)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        d = _code_plane(_pad(d, 8, 8), tc)[:h2, :w2]
        if w2 <= 2:  # jdsample.c: the fancy upsampler needs more than two columns; below that, replication
            u = np.repeat(np.repeat(d, 2, 0), 2, 1)
        else:
            up = np.pad(d, ((1, 1), (0, 0)), mode="edge")
            near = np.repeat(d, 2, axis=0)
            far = np.empty_like(near)
            far[0::2], far[1::2] = up[:-2], up[2:]
            cs = 3 * near + far
            last = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
            nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
            u = np.empty((2 * h2, 2 * w2), i32)
            u[:, 0::2] = (3 * cs + last + 8) >> 4
            u[:, 1::2] = (3 * cs + nxt + 7) >> 4
        dec.append(u[:h, :w] - 128)
    cb, cr = dec
    rr = yd + ((fix(1.402) * cr + half) >> 16)
    gg = yd + ((-fix(.34414) * cb + half - fix(.71414) * cr) >> 16)
    bb = yd + ((fix(1.772) * cb + half) >> 16)
    return np.clip(np.stack([rr, gg, bb], -1), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- inputs and the case grid
# the smallest shapes at which each rule can go wrong: one whole MCU; chroma width 4 (padding before the
# downsampling); odd both ways; one pixel; a height below one block with chroma width 25; an odd pair; the small
# output of the chain tests; chroma widths 2 and 1 (the replicating upsampler); the LDS-resident size
SHAPES = ((16, 16), (8, 8), (9, 9), (1, 1), (7, 50), (17, 23), (24, 20), (9, 4), (5, 2), (224, 224))
CONTENTS = ("noise", "ramp", "sat")
QUALITIES = (35, 50, 75, 95)
EXTREME = {(16, 16): (1, 100), (9, 9): (1, 100)}
GOLDEN_ROWS = (0, 111, 223)  # what a 224 x 224 case stores next to its checksum


def source(shape, content):
    """uniform noise, a smooth ramp, or saturated 0 / 255 noise; RandomState's stream is frozen"""
    h, w = shape
    rs = np.random.RandomState(1000 * h + 10 * w + CONTENTS.index(content))
    if content == "noise":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "sat":
        return (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 5 + xx * 3) % 256, (xx * 7) % 256, (yy * 2 + 40 + xx // 3) % 256], -1).astype(np.uint8)


def digest(a):
    return np.array([zlib.crc32(np.ascontiguousarray(a).tobytes())], np.uint32)


def src_key(shape, content):
    return f"{shape[0]}x{shape[1]}/{content}"


def cases():
    """-> [(name, shape, content, quality)]"""
    out = []
    for shape in SHAPES:
        for content in CONTENTS:
            for q in QUALITIES + EXTREME.get(shape, ()):
                out.append((f"{src_key(shape, content)}/q{q}", shape, content, q))
    return out
