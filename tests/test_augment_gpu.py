"""``torch.ops.dfd.augment_frames`` (``csrc/k_augment.hip``) on the device.

Single-stage cases against Pillow's results (``tests/golden/augment.npz``) with the host test's bounds (exact;
the blur within one code value of ``conv2d``), whole chains -- all stages on at 224 x 224 with N = 5 (the
LDS-resident path), odd sizes, and an output too large for LDS (the scratch path) -- against the numpy
restatement with exact equality, the identity, ``resize_frames``, the input and table guards,
``torch.library.opcheck`` and ``TrainAugment`` on a ``collate_clips`` batch.  Cases of one (source, output)
shape share one launch, so a launch carries rows with different stages."""
import numpy as np
import pytest
import torch

import augment_helpers as ah
from deepfake_amd import _lib, augment, ops
from deepfake_amd.pipeline import collate_clips
from test_augment_host import CASES, GOLD, check_against_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sources():
    return {name: ah.source(name) for name in ah.SOURCES}


def run(cuda, a, pis, pfs, out_hw):
    """one source frame under every row of the tables -> (N, oh, ow, 3) numpy"""
    pis, pfs = np.atleast_2d(pis), np.atleast_2d(pfs)
    src = torch.from_numpy(a).to(cuda).expand(len(pis), *a.shape).contiguous()
    out = augment.augment_frames(src, torch.from_numpy(pis), torch.from_numpy(pfs), out_hw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(pis), *out_hw, 3) and out.device == src.device
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def grid_results(cuda, sources):
    """every single-stage case, one launch per (source, output shape)"""
    groups = {}
    for c in CASES:
        groups.setdefault((c[1], c[2]), []).append(c)
    res = {}
    for (src, out_hw), cs in groups.items():
        got = run(cuda, sources[src], np.stack([c[3] for c in cs]), np.stack([c[4] for c in cs]), out_hw)
        for c, g in zip(cs, got):
            res[c[0]] = g
    return res


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stage_matches_pillow(case, grid_results):
    check_against_golden(case[0], grid_results[case[0]], case[3])


@pytest.mark.parametrize("case", ah.composed_cases(), ids=[c[0] for c in ah.composed_cases()])
def test_chain_equals_restatement(case, cuda, sources):
    name, src, out_hw, pis, pfs = case
    got = run(cuda, sources[src], pis, pfs, out_hw)
    for n, (pi, pf) in enumerate(zip(pis, pfs)):
        want = ah.chain(sources[src], pi, pf, out_hw)
        bad = int((got[n] != want).sum())
        assert bad == 0, (f"{name}, frame {n}: {bad} bytes differ, max "
                          f"{int(np.abs(got[n].astype(int) - want.astype(int)).max())}")


def test_paths():
    lib = _lib.load()
    assert lib.dfd_augment_lds_resident(224, 224, 224, 224) == 1  # 150,528 B image + 12,544 B tables
    assert lib.dfd_augment_lds_resident(37, 41, 24, 20) == 1
    assert lib.dfd_augment_lds_resident(224, 224, 300, 260) == 0
    assert lib.dfd_augment_lds_resident(0, 224, 224, 224) == -1


def test_all_off_is_the_identity(cuda, sources):
    for name in ("odd", "full"):
        a = sources[name]
        pi, pf = augment.identity_params(3, a.shape[:2])
        src = torch.from_numpy(np.stack([a, a[::-1].copy(), a[:, ::-1].copy()])).to(cuda)
        out = augment.augment_frames(src, pi, pf, a.shape[:2])
        assert torch.equal(out, src)


def test_resize_frames_equals_golden(cuda, sources):
    for name, src, out_hw in (("resize/odd/24x20/whole", "odd", (24, 20)), ("resize/full/41x37/whole", "full", (41, 37)),
                              ("resize/odd/224x224/whole", "odd", (224, 224))):
        got = augment.resize_frames(torch.from_numpy(sources[src][None]).to(cuda), out_hw).cpu().numpy()[0]
        check_against_golden(name, got, np.zeros(ah.PI, np.int32))


def test_guards(cuda, sources):
    a = sources["odd"]
    h, w = a.shape[:2]
    src = torch.from_numpy(a[None]).to(cuda)
    pi, pf = augment.identity_params(1, (h, w))
    with pytest.raises(RuntimeError):  # non-contiguous frames
        augment.augment_frames(torch.from_numpy(np.stack([a, a])).to(cuda)[:, :, ::2], pi.repeat(2, 1), pf.repeat(2, 1),
                               (h, w))
    with pytest.raises(RuntimeError):  # float frames
        augment.augment_frames(src.float(), pi, pf, (h, w))
    with pytest.raises(RuntimeError):  # NCHW frames
        augment.augment_frames(src.permute(0, 3, 1, 2).contiguous(), pi, pf, (h, w))
    with pytest.raises(RuntimeError):  # tables of the wrong type / shape
        augment.augment_frames(src, pi.long(), pf, (h, w))
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi, pf.double(), (h, w))
    with pytest.raises(RuntimeError):
        augment.augment_frames(src, pi.repeat(2, 1), pf.repeat(2, 1), (h, w))
    with pytest.raises(_lib.DFDError):  # frames on the host: no CPU path
        augment.augment_frames(src.cpu(), pi, pf, (h, w))
    with pytest.raises(NotImplementedError):
        torch.ops.dfd.augment_frames(src.cpu(), pi, pf, [h, w])

    def bad(col, value, table="i", flags=0):
        qi, qf = pi.clone(), pf.clone()
        qi[0, 0] = flags
        (qi if table == "i" else qf)[0, col] = value
        assert not ah.valid_row(qi[0].numpy(), qf[0].numpy(), (h, w), (h, w))
        with pytest.raises(_lib.DFDError, match="augment_frames: frame 0"):
            augment.augment_frames(src, qi, qf, (h, w))

    bad(3, h + 1)  # box taller than the source
    bad(2, 1)  # full-width box moved right
    bad(1, -1)
    bad(4, 0)
    bad(6, 0)  # permutation with a repeat
    bad(8, 4)
    bad(9, 256)
    bad(10, 0, flags=ah.DOWNUP)
    bad(11, 0)
    bad(11, w + 1)
    bad(0, 32)
    bad(1, float("nan"), table="f")
    with pytest.raises(_lib.DFDError, match="blur needs"):
        qi, qf = augment.identity_params(1, (h, w), (1, 5))
        qi[0, 0] = ah.BLUR
        augment.augment_frames(src, qi, qf, (1, 5))
    torch.cuda.synchronize()


def test_opcheck(cuda, sources):
    a = sources["odd"]
    _n, _s, out_hw, pis, pfs = ah.composed_cases()[0]
    src = torch.from_numpy(np.stack([a] * len(pis))).to(cuda)
    assert "augment_frames" in ops.AUGMENT_OPS
    torch.library.opcheck(torch.ops.dfd.augment_frames.default,
                          (src, torch.from_numpy(pis), torch.from_numpy(pfs), list(out_hw)))


def test_train_augment_on_a_collated_batch(cuda, sources):
    a = sources["odd"]
    h, w = a.shape[:2]
    batch = [{"faces": np.stack([a, a[::-1].copy(), a[:, ::-1].copy()]), "label": 1},
             {"faces": np.stack([a[::-1, ::-1].copy()]), "label": 0}]
    x, labels = collate_clips(batch, max_frames=3, image_size=(h, w), device=cuda, out="uint8")
    aug = augment.TrainAugment((24, 20), torch.Generator().manual_seed(3))
    y = aug(x)
    assert y.dtype == torch.uint8 and tuple(y.shape) == (2, 3, 3, 24, 20) and y.device == x.device
    assert y.stride() == y.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3).stride()  # channels-last
    pi, pf = augment.draw_augment_params(6, (h, w), (24, 20), torch.Generator().manual_seed(3))
    frames = x.permute(0, 1, 3, 4, 2).reshape(6, h, w, 3).cpu().numpy()
    for n in range(6):
        want = ah.chain(frames[n], pi[n].numpy(), pf[n].numpy(), (24, 20))
        assert np.array_equal(y.permute(0, 1, 3, 4, 2).reshape(6, 24, 20, 3)[n].cpu().numpy(), want), n
