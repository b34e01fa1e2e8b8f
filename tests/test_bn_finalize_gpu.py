"""The train-mode BatchNorm finalize from centred tile partials, plain and chunked (``k_bn.hip``).

``dfd_rn_bn_train_finalize`` hands ``launch_bn_finalize`` rows of (tile sum, tile M2) over 64-row
tiles.  Up to 4 x 512 rows one kernel reduces them (``bn_finalize_kernel``: the between-tile term from a
second pass once the mean is known); above that the single-pass chunked form runs
(``bn_chan_chunks_kernel`` + ``bn_chan_final_kernel``), whose fp64 chunk partials live in a scratch
buffer kept per (device, stream) and grown on demand.  Both sides of the threshold are checked here:

* rows = 2048 (plain) and 2049 (the first chunked row count: five chunks, the last of one row);
* C = 72: not a multiple of the chunk kernel's 64 channels per workgroup, so its ``c < C`` guard and its
  second ``blockIdx.y`` are live;
* count = 64 * rows - 17: the last tile is short;
* on a non-default stream, 2049 rows twice, C = 72 then C = 144: the scratch lookup and its grow path.

The reference is Chan's merge of the same fp32 rows in float64 (numpy).  Tolerance: what
``test_resnet_train_gpu.py`` asks of the BatchNorm running buffers (rtol 1e-4, atol 1e-5), here for
mean / invstd / scale / shift and the updated running pair alike.
"""
import numpy as np
import pytest
import torch

import deepfake_amd  # noqa: F401
from deepfake_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 64  # kConvStatRows
SHORT = 17  # elements missing from the last tile
CMAX = 144
RTOL, ATOL = 1e-4, 1e-5
MOMENTUM, EPS = 0.1, 1e-5

_ROWS = {}


def _stat_rows(rows):
    """fp32 [rows][2][CMAX] (tile sum, tile M2 about the tile's own mean) of seeded fp32 data (cached)"""
    if rows not in _ROWS:
        g = torch.Generator().manual_seed(100 + rows)
        x = torch.randn(rows * TILE, CMAX, generator=g)
        x = x * (0.5 + torch.rand(CMAX, generator=g)) + torch.randn(CMAX, generator=g)
        x = x.view(rows, TILE, CMAX).double()
        nt = torch.full((rows,), float(TILE), dtype=torch.float64)
        nt[-1] = TILE - SHORT
        valid = (torch.arange(TILE)[None, :] < nt[:, None])[:, :, None]
        s = (x * valid).sum(1)
        m2 = (((x - (s / nt[:, None])[:, None, :]) ** 2) * valid).sum(1)
        _ROWS[rows] = torch.stack([s, m2], 1).float().numpy()
    return _ROWS[rows]


def _merge(st, count, gamma, beta, rm, rv):
    """Chan's merge of the tiles in float64 and the constants / running update that follow"""
    st = st.astype(np.float64)
    rows = st.shape[0]
    nt = np.full(rows, float(TILE))
    nt[-1] = count - TILE * (rows - 1)
    mean = st[:, 0].sum(0) / count
    var = (st[:, 1].sum(0) + (nt[:, None] * (st[:, 0] / nt[:, None] - mean) ** 2).sum(0)) / count
    invstd = 1.0 / np.sqrt(var + EPS)
    scale = gamma * invstd
    return dict(mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale,
                running_mean=(1.0 - MOMENTUM) * rm + MOMENTUM * mean,
                running_var=(1.0 - MOMENTUM) * rv + MOMENTUM * var * count / (count - 1))


def _check(cuda, rows, C, stream=None):
    lib = _lib.load()
    count = TILE * rows - SHORT
    st = np.ascontiguousarray(_stat_rows(rows)[:, :, :C])
    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ref = _merge(st, count, *(t.double().numpy() for t in (gamma, beta, rm, rv)))
    d_st, d_g, d_b, d_rm, d_rv = (t.to(cuda) for t in (torch.from_numpy(st), gamma, beta, rm, rv))
    out = torch.zeros(4, C, device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(cuda)):
        _lib.check(lib.dfd_rn_bn_train_finalize(_lib.stream_of(cuda), d_st.data_ptr(), rows, count, C, d_g.data_ptr(),
                                                d_b.data_ptr(), d_rm.data_ptr(), d_rv.data_ptr(), MOMENTUM, EPS,
                                                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                out[3].data_ptr()))
    torch.cuda.synchronize()
    got = dict(mean=out[0], invstd=out[1], scale=out[2], shift=out[3], running_mean=d_rm, running_var=d_rv)
    for name, r in ref.items():
        a = got[name].double().cpu().numpy()
        print(f"rows {rows} C {C} {name}: max |diff| {np.abs(a - r).max():.3e}, max rel "
              f"{(np.abs(a - r) / (np.abs(r) + 1e-30)).max():.3e}")
        np.testing.assert_allclose(a, r, rtol=RTOL, atol=ATOL, err_msg=f"rows {rows} C {C} {name}")


@pytest.mark.parametrize("rows", [2048, 2049])
def test_finalize_plain_and_chunked(cuda, rows):
    _check(cuda, rows, 72)


def test_chunked_scratch_reuse_and_grow(cuda):
    side = torch.cuda.Stream(cuda)
    _check(cuda, 2049, 72, side)
    _check(cuda, 2049, CMAX, side)
