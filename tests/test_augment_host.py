"""CPU checks of the augmentation chain's restatement and of the host-side draw (no GPU, no launch).

``tests/augment_helpers.py`` restates every stage of ``csrc/k_augment.hip`` in numpy; here each stage is held
to Pillow's results (``tests/golden/augment.npz``): exact equality for resize, flip, brightness, contrast,
saturation, grayscale and downscale/upscale; hue exact as well, since the restated HSV conversions differ
from Pillow 12.2.0's by 0 over all 2^24 colours (recorded in the fixture); the blur within one code value of
``conv2d``, whose summation order is its own."""
import numpy as np
import pytest
import torch

import augment_helpers as ah
from deepfake_amd import augment

GOLD = np.load(ah.__file__.replace("augment_helpers.py", "golden/augment.npz"))
CASES = ah.cases()


@pytest.fixture(scope="module")
def sources():
    s = {name: ah.source(name) for name in ah.SOURCES}
    for name in ("odd", "tiny"):
        assert np.array_equal(s[name], GOLD[f"src/{name}"]), "the seeded source no longer matches the fixture's"
    return s


def bound(pi):
    return 1 if pi[0] & ah.BLUR else 0


def check_against_golden(name, got, pi):
    """whole frame, or checksum + rows for a 224 x 224 case; the blur's bound is one code value"""
    if f"out/{name}" in GOLD:
        want = GOLD[f"out/{name}"]
        d = int(np.abs(got.astype(int) - want.astype(int)).max())
        assert got.shape == want.shape and d <= bound(pi), f"{name}: max difference {d}"
        return
    rows = GOLD[f"rows/{name}"]
    d = int(np.abs(got[list(ah.GOLDEN_ROWS)].astype(int) - rows.astype(int)).max())
    assert d <= bound(pi), f"{name}: max difference {d} on the stored rows"
    if bound(pi) == 0:
        assert ah.digest(got)[0] == GOLD[f"crc/{name}"][0], f"{name}: checksum differs"


def test_hue_restatement_is_exact_against_pillow():
    assert GOLD["hsv_max_diff"].tolist() == [0, 0] and str(GOLD["pillow_version"]) == "12.2.0"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_pillow(case, sources):
    name, src, out_hw, pi, pf, _s, _sigma = case
    check_against_golden(name, ah.chain(sources[src], pi, pf, out_hw), pi)


def test_grid_covers_the_issue():
    names = [c[0] for c in CASES]
    for stage in ("resize", "flip", "brightness", "contrast", "saturation", "hue", "gray", "downup", "blur"):
        assert sum(n.startswith(stage + "/") for n in names) >= 2 or stage == "gray", stage
    assert sum(n.startswith("jitter/") for n in names) >= 4
    tiny = [c for c in CASES if c[0] == "downup/tiny/0.55"][0]
    assert tuple(tiny[3][10:12]) == (8, 8)  # max(8, int(12 * .55)), max(8, int(10 * .55)): both clamp
    for _n, src, out_hw, pi, pf, _s, _g in CASES:
        assert ah.valid_row(pi, pf, ah.SOURCES[src][:2], out_hw)
    for _n, src, out_hw, pis, pfs in ah.composed_cases():
        assert all(ah.valid_row(a, b, ah.SOURCES[src][:2], out_hw) for a, b in zip(pis, pfs))


def test_identity_chain(sources):
    a = sources["odd"]
    pi, pf = augment.identity_params(1, a.shape[:2])
    assert np.array_equal(ah.chain(a, pi[0].numpy(), pf[0].numpy(), a.shape[:2]), a)


# ---------------------------------------------------------------- draw_augment_params
def draw(n=400, src=(224, 200), out=(224, 224), seed=5, **kw):
    g = torch.Generator().manual_seed(seed)
    pi, pf = augment.draw_augment_params(n, src, out, g, **kw)
    return pi.numpy(), pf.numpy()


def test_draw_is_reproducible_and_typed():
    a, b = draw(), draw()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = draw(seed=6)
    assert not np.array_equal(a[0], c[0])
    assert a[0].dtype == np.int32 and a[0].shape == (400, ah.PI) and a[1].dtype == np.float32 and a[1].shape == (400, ah.PF)


def test_draw_boxes_and_ranges():
    h, w = 224, 200
    pi, pf = draw()
    i, j, bh, bw = pi[:, 1], pi[:, 2], pi[:, 3], pi[:, 4]
    assert (i >= 0).all() and (j >= 0).all() and (i + bh <= h).all() and (j + bw <= w).all() and (bh > 0).all()
    # get_params rounds sqrt(area * ratio) and sqrt(area / ratio) to integers: half a pixel each way
    fallback = (bw == w) & (bh == int(round(w / 0.9)))  # 200 / 224 < 0.9: full width, ratio 0.9
    area_lo, area_hi = (bw - 0.5) * (bh - 0.5) / (h * w), (bw + 0.5) * (bh + 0.5) / (h * w)
    ratio_lo, ratio_hi = (bw - 0.5) / (bh + 0.5), (bw + 0.5) / (bh - 0.5)
    ok = (area_hi >= 0.75) & (area_lo <= 1.0) & (ratio_hi >= 0.9) & (ratio_lo <= 1.1)
    assert (ok | fallback).all()
    assert (ok & ~fallback).sum() > 300  # the tries mostly succeed at this shape
    assert all(sorted(r) == [0, 1, 2, 3] for r in pi[:, 5:9].tolist())
    assert len({tuple(r) for r in pi[:, 5:9].tolist()}) > 12  # of the 24 orders
    assert (np.abs(pf[:, 3:6].sum(1) - 1) <= 3 * np.finfo(np.float32).eps).all()
    assert (pf[:, 3] == pf[:, 5]).all() and (pf[:, 4] >= pf[:, 3]).all()
    assert (pf[:, 0] >= 0.75).all() and (pf[:, 0] <= 1.25).all() and (pf[:, 2] >= 0.8).all() and (pf[:, 2] <= 1.2).all()
    assert set(pi[:, 9].tolist()) <= {0, 1, 2, 3, 4, 5, 251, 252, 253, 254, 255}
    s_lo, s_hi = int(224 * 0.55), int(224 * 0.9)
    assert (pi[:, 10] >= s_lo).all() and (pi[:, 10] <= s_hi).all() and (pi[:, 11] >= s_lo).all()
    assert all(ah.valid_row(a, b, (h, w), (224, 224)) for a, b in zip(pi, pf))
    # the flags come at roughly their probabilities (400 draws: 5 sigma)
    for bit, p in ((ah.FLIP, 0.5), (ah.JITTER, 0.7), (ah.GRAY, 0.05), (ah.DOWNUP, 0.25), (ah.BLUR, 0.25)):
        assert abs(((pi[:, 0] & bit) != 0).mean() - p) <= 5 * (p * (1 - p) / 400) ** 0.5, bit


def test_draw_fallback_is_the_centre_crop():
    # a 10 x 100 source can hold no box of ratio 0.9-1.1 and 75 % of the area: every row is the fallback
    pi, pf = draw(n=20, src=(10, 100), out=(16, 16))
    assert (pi[:, 3] == 10).all() and (pi[:, 4] == 11).all() and (pi[:, 1] == 0).all() and (pi[:, 2] == 44).all()
    assert all(ah.valid_row(a, b, (10, 100), (16, 16)) for a, b in zip(pi, pf))
    assert (pi[:, 10:12] >= 8).all() and (pi[:, 10:12] <= 14).all()  # max(8, int(16 * s)), s in [0.55, 0.9)


def test_draw_blur_taps_match_torchvision_formula():
    for sigma in (0.1, 0.7, 2.0):
        k = augment.blur_taps(sigma)
        assert np.array_equal(k, ah.blur_taps(sigma)) and k.dtype == np.float32
