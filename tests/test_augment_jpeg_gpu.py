"""``torch.ops.dfd.augment_frames_jpeg`` (the JPEG stage of ``csrc/k_augment.hip``) on the device.

The stage alone against Pillow's bytes (``tests/golden/augment_jpeg.npz``) on every case of the grid, launches that
mix frames with and without the stage against ``augment_frames``, whole chains -- (24, 20) from the odd source,
224 x 224 (the LDS-resident path) and an output too large for LDS (the scratch path) -- against the numpy
restatement, the guards, ``torch.library.opcheck`` and ``TrainAugment(jpeg=True)`` on a ``collate_clips`` batch.
Every comparison is exact equality.  Cases of one shape share a launch, so a launch carries different
qualities."""
import numpy as np
import pytest
import torch

import augment_helpers as ah
import jpeg_helpers as jh
from deepfake_amd import _lib, augment, ops
from deepfake_amd.pipeline import collate_clips
from test_augment_jpeg_host import CASES, IDS, check_against_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sources():
    return {name: ah.source(name) for name in ah.SOURCES}


def qt(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int32)


def run(cuda, frames, pis, pfs, quality, out_hw):
    """frames (N, H, W, 3) numpy under the rows of the tables and the qualities -> (N, oh, ow, 3) numpy"""
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(cuda)
    out = augment.augment_frames(src, torch.from_numpy(np.atleast_2d(pis)), torch.from_numpy(np.atleast_2d(pfs)),
                                 out_hw, qt(quality))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(frames), *out_hw, 3) and out.device == src.device
    return out.cpu().numpy()


def identity(n, hw):
    pi, pf = augment.identity_params(n, hw)
    return pi.numpy(), pf.numpy()


@pytest.fixture(scope="module")
def grid_results(cuda):
    """every grid case with only the JPEG stage on (identity tables, source = output size), one launch per shape"""
    res = {}
    for shape in jh.SHAPES:
        cs = [c for c in CASES if c[1] == shape]
        frames = np.stack([jh.source(shape, c[2]) for c in cs])
        pi, pf = identity(len(cs), shape)
        got = run(cuda, frames, pi, pf, [c[3] for c in cs], shape)
        for c, g in zip(cs, got):
            res[c[0]] = g
    return res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stage_matches_pillow(case, grid_results):
    check_against_golden(case[0], grid_results[case[0]])


def test_quality_zero_rows_equal_the_plain_op(cuda, sources):
    # a launch that mixes frames with and without the stage
    name, src, out_hw, pis, pfs = ah.composed_cases()[0]
    a = sources[src]
    pis, pfs = np.concatenate([pis, pis]), np.concatenate([pfs, pfs])
    quality = [0, 75, 0, 35, 0, 95]
    frames = np.stack([a] * len(pis))
    got = run(cuda, frames, pis, pfs, quality, out_hw)
    plain = torch.ops.dfd.augment_frames(torch.from_numpy(frames).to(cuda), torch.from_numpy(pis),
                                         torch.from_numpy(pfs), list(out_hw)).cpu().numpy()
    for n, q in enumerate(quality):
        assert np.array_equal(got[n], plain[n]) == (q == 0), n
    # all qualities 0: the old op, on every composed case (LDS and scratch paths)
    for name, src, out_hw, pis, pfs in ah.composed_cases():
        frames = np.stack([sources[src]] * len(pis))
        got = run(cuda, frames, pis, pfs, [0] * len(pis), out_hw)
        plain = torch.ops.dfd.augment_frames(torch.from_numpy(frames).to(cuda), torch.from_numpy(pis),
                                             torch.from_numpy(pfs), list(out_hw)).cpu().numpy()
        assert np.array_equal(got, plain), name


def restated(a, pi, pf, q, out_hw):
    """the whole chain with the JPEG stage between the downscale/upscale and the blur"""
    x = ah.chain(a, pi, pf, out_hw, stages=ah.ALL & ~ah.BLUR)
    x = jh.jpeg_roundtrip(x, q)
    return ah.blur(x, pf[3:6]) if int(pi[0]) & ah.BLUR else x


def all_on_rows(src_hw, out_hw, n):
    rows = [ah.row(src_hw, out_hw, box=(1 + k, 2 * k, src_hw[0] - 4 - k, src_hw[1] - 5 - k),
                   flags=ah.ALL & ~(ah.GRAY if k % 2 else 0),
                   perm=((2, 3, 1, 0), (3, 0, 2, 1), (0, 1, 2, 3), (1, 2, 3, 0))[k % 4],
                   factors=(0.8 + 0.12 * k, 1.25 - 0.1 * k, 0.85 + 0.1 * k), hue_f=-0.02 + 0.012 * k,
                   s=0.55 + 0.1 * k, sigma=0.4 + 0.5 * k) for k in range(n)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@pytest.mark.parametrize("src,out_hw,quality", [("odd", (24, 20), (35, 95, 50, 75)), ("full", (224, 224), (75, 35, 95)),
                                                ("full", (300, 260), (60, 0))],
                         ids=["odd->24x20", "full->224x224 (LDS)", "full->300x260 (scratch path)"])
def test_chain_with_jpeg_equals_restatement(src, out_hw, quality, cuda, sources):
    a = sources[src]
    pis, pfs = all_on_rows(a.shape[:2], out_hw, len(quality))
    assert all(ah.valid_row(p, f, a.shape[:2], out_hw) and int(p[0]) & ah.DOWNUP and int(p[0]) & ah.BLUR
               for p, f in zip(pis, pfs))
    assert _lib.load().dfd_augment_lds_resident(*a.shape[:2], *out_hw) == (0 if out_hw == (300, 260) else 1)
    got = run(cuda, np.stack([a] * len(quality)), pis, pfs, quality, out_hw)
    for n, q in enumerate(quality):
        want = restated(a, pis[n], pfs[n], q, out_hw)
        bad = int((got[n] != want).sum())
        assert bad == 0, (f"frame {n} (quality {q}): {bad} bytes differ, max "
                          f"{int(np.abs(got[n].astype(int) - want.astype(int)).max())}")


def test_guards(cuda):
    shape = (17, 23)
    a = jh.source(shape, "noise")
    src = torch.from_numpy(np.stack([a, a])).to(cuda)
    pi, pf = augment.identity_params(2, shape)
    for bad in (qt([75, 101]), qt([-1, 75])):
        with pytest.raises(_lib.DFDError, match="augment_frames: frame"):
            augment.augment_frames(src, pi, pf, shape, bad)
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi, pf, shape, torch.tensor([75.0, 75.0]))
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi, pf, shape, torch.tensor([75, 75], dtype=torch.int64))
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi, pf, shape, qt([75]))
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi, pf, shape, qt([75, 75, 75]))
    qi = pi.clone()
    qi[1, 0] = 32  # the quality is no flag: bit 32 stays unknown on both entries
    with pytest.raises(_lib.DFDError, match="augment_frames: frame 1"):
        augment.augment_frames(src, qi, pf, shape, qt([75, 75]))
    # nothing was enqueued by the failures, and a valid call still returns the right bytes
    got = augment.augment_frames(src, pi, pf, shape, qt([75, 0])).cpu().numpy()
    check_against_golden("17x23/noise/q75", got[0])
    assert np.array_equal(got[1], a)


def test_opcheck(cuda, sources):
    a = sources["odd"]
    _n, _s, out_hw, pis, pfs = ah.composed_cases()[0]
    src = torch.from_numpy(np.stack([a] * len(pis))).to(cuda)
    assert "augment_frames_jpeg" in ops.AUGMENT_OPS
    torch.library.opcheck(torch.ops.dfd.augment_frames_jpeg.default,
                          (src, torch.from_numpy(pis), torch.from_numpy(pfs), qt([75, 0, 40]), list(out_hw)))


def test_train_augment_with_jpeg_on_a_collated_batch(cuda, sources):
    a = sources["odd"]
    h, w = a.shape[:2]
    batch = [{"faces": np.stack([a, a[::-1].copy(), a[:, ::-1].copy()]), "label": 1},
             {"faces": np.stack([a[::-1, ::-1].copy()]), "label": 0}]
    x, _labels = collate_clips(batch, max_frames=3, image_size=(h, w), device=cuda, out="uint8")
    y = augment.TrainAugment((24, 20), torch.Generator().manual_seed(3), jpeg=True)(x)
    assert y.dtype == torch.uint8 and tuple(y.shape) == (2, 3, 3, 24, 20) and y.device == x.device
    g = torch.Generator().manual_seed(3)
    pi, pf = augment.draw_augment_params(6, (h, w), (24, 20), g)
    q = augment.draw_jpeg_quality(6, g)
    assert (q != 0).any()
    frames = x.permute(0, 1, 3, 4, 2).reshape(6, h, w, 3).cpu().numpy()
    got = y.permute(0, 1, 3, 4, 2).reshape(6, 24, 20, 3).cpu().numpy()
    for n in range(6):
        assert np.array_equal(got[n], restated(frames[n], pi[n].numpy(), pf[n].numpy(), int(q[n]), (24, 20))), n
    plain = augment.TrainAugment((24, 20), torch.Generator().manual_seed(3))(x)
    plain = plain.permute(0, 1, 3, 4, 2).reshape(6, 24, 20, 3).cpu().numpy()
    differs = [not np.array_equal(got[n], plain[n]) for n in range(6)]
    assert any(differs) and all(int(q[n]) != 0 for n, d in enumerate(differs) if d)
