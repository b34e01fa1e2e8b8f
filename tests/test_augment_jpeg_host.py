"""CPU checks of the JPEG stage's restatement and of its host-side draw (no GPU, no launch).

``tests/jpeg_helpers.py`` restates libjpeg-turbo's baseline 4:2:0 round trip in 32-bit numpy integers; here it
is held to the bytes the reference's ``_RandomJPEGCompression`` produced with Pillow 12.2.0
(``tests/golden/augment_jpeg.npz``) with exact equality on every case of the grid, and, where Pillow is
installed, to a live round trip as well."""
import io
import os

import numpy as np
import pytest
import torch

import augment_helpers as ah
import jpeg_helpers as jh
from deepfake_amd import augment

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(jh.__file__)), "golden", "augment_jpeg.npz"))
CASES = jh.cases()
IDS = [c[0] for c in CASES]


def check_against_golden(name, got):
    """whole frame, or checksum + rows for a 224 x 224 case; 0 differing bytes"""
    if f"out/{name}" in GOLD:
        want = GOLD[f"out/{name}"]
        assert got.shape == want.shape and got.dtype == np.uint8
        bad = int((got != want).sum())
        assert bad == 0, f"{name}: {bad} bytes differ, max {int(np.abs(got.astype(int) - want.astype(int)).max())}"
        return
    rows = GOLD[f"rows/{name}"]
    bad = int((got[list(jh.GOLDEN_ROWS)] != rows).sum())
    assert bad == 0, f"{name}: {bad} bytes differ on the stored rows"
    assert jh.digest(got)[0] == GOLD[f"crc/{name}"][0], f"{name}: checksum differs"


def test_fixture_and_grid():
    assert str(GOLD["pillow_version"]) == "12.2.0" and int(GOLD["libjpeg_turbo"][0]) == 1
    shapes = {c[1] for c in CASES}
    assert {(16, 16), (8, 8), (9, 9), (1, 1), (7, 50), (17, 23), (24, 20), (224, 224)} <= shapes
    for shape in shapes:
        for content in ("noise", "ramp", "sat"):
            qs = {c[3] for c in CASES if c[1] == shape and c[2] == content}
            assert {35, 50, 75, 95} <= qs
            if shape in ((16, 16), (9, 9)):
                assert {1, 100} <= qs
            if shape != (224, 224):
                assert np.array_equal(jh.source(shape, content), GOLD[f"src/{jh.src_key(shape, content)}"]), \
                    "the seeded source no longer matches the fixture's"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_matches_fixture(case):
    name, shape, content, q = case
    check_against_golden(name, jh.jpeg_roundtrip(jh.source(shape, content), q))


def test_restatement_matches_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    for name, shape, content, q in CASES:
        if shape == (224, 224) and content != "noise":
            continue
        a = jh.source(shape, content)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=q, optimize=True)
        buf.seek(0)
        want = np.array(Image.open(buf).convert("RGB"))
        assert np.array_equal(jh.jpeg_roundtrip(a, q), want), name


def test_quality_zero_is_a_copy():
    a = jh.source((9, 9), "noise")
    assert np.array_equal(jh.jpeg_roundtrip(a, 0), a)


# ---------------------------------------------------------------- draw_jpeg_quality
def draw(n=4000, seed=7, **kw):
    return augment.draw_jpeg_quality(n, torch.Generator().manual_seed(seed), **kw)


def test_draw_jpeg_quality():
    a, b = draw(), draw()
    assert a.dtype == torch.int32 and tuple(a.shape) == (4000,) and a.device.type == "cpu"
    assert torch.equal(a, b) and not torch.equal(a, draw(seed=8))
    q = a.numpy()
    on = q != 0
    assert ((q[on] >= 35) & (q[on] <= 95)).all()
    assert (q == 35).any() and (q == 95).any()  # randint: both ends inclusive
    assert abs(on.mean() - 0.5) <= 5 * (0.25 / 4000) ** 0.5
    assert not draw(p=0.0).any()
    assert (draw(p=1.0, quality=(60, 60)) == 60).all()


def test_quality_draw_leaves_the_tables_alone():
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    pi1, pf1 = augment.draw_augment_params(50, (37, 41), (24, 20), g1)
    pi2, pf2 = augment.draw_augment_params(50, (37, 41), (24, 20), g2)
    q = augment.draw_jpeg_quality(50, g2)
    assert torch.equal(pi1, pi2) and torch.equal(pf1, pf2) and tuple(q.shape) == (50,)
    assert pi1.shape[1] == ah.PI and pf1.shape[1] == ah.PF
    # and the quality comes from the draws that follow the tables' on the same stream
    g3 = torch.Generator().manual_seed(11)
    torch.rand(50, 37, dtype=torch.float64, generator=g3)
    assert torch.equal(q, augment.draw_jpeg_quality(50, g3))
