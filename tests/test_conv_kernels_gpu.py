"""The fp32 convolution launchers of ``csrc/k_conv.hip`` (``conv_forward`` / ``conv_dgrad`` / ``conv_wgrad``)
through the ``dfd_test_conv_*`` seam, at the templates only CNNLSTMHybrid uses (``fold = 0``, with a conv
bias) and at the smallest shapes where the persistent tile grid wraps, for ``fold = 0`` and ``fold = 1``.

Reference: ``F.conv2d`` and its autograd in fp64 on the same fp32 operands, plain PyTorch on the GPU with
MIOpen off (as ``test_resnet_train_gpu.py``), a few images at a time.  Judged like the gradients of
``cnn_lstm_helpers.py``: err_hip <= K_CL x max(err_torch_fp32, CONV_FLOOR), errors relative L2 against
fp64, torch's own fp32 ``conv2d`` / autograd on the same chunks as the anchor -- for the whole tensor, the
worst pixel row and the worst channel of y and dx, and the whole tensor and the worst dim-0 row of dw (row
denominators floored at 5 % of the median row norm, as ``b0_helpers.grad_errors``).  CONV_FLOOR = 2^-24,
the fp32 unit roundoff: every output element is rounded to fp32 at least once.  The forward's 64-row BN
partials (sum, M2 about the tile mean) of y + bias are held to the fp64 y at the ResNet test's bounds.

Launch arithmetic (k_conv.hip; M = output pixels for forward / wgrad, input pixels for dgrad; cg32 =
the wide-vector tile loops, taken when Cin, Cout % 64 == 0 over dense NHWC; gx = min(tiles_m, 1024 / ntn)
workgroups per tile column; wgrad: sp = min(512 / tiles, cdiv(M, 128), slab / |dw|) M-splits of
mps = 128-row multiples, one workgroup per (64 x 64 tile, split) -- the weight gradient has no persistent
loop, its edges are the ragged last split and the slab-capped split count):

``LAYERS`` -- the model's four geometries at odd non-square maps, N = 3, fold = 0, bias:
  stem   3->64 7x7/2 on 37x51 (-> 19x26, M = 1482), read through channels-last strides and again through
         plain NCHW strides: conv_gemm<OpConvA> 64x64 tiles (24 row tiles, the last of 10 rows), wgrad
         conv_gemm<OpCols, OpConvBT> in min(cdiv(M, 256), 2048 / 3) = 6 pixel splits; no dgrad (an input)
  c2     64->128 5x5 on 19x13 (M = 741): cg32_fwd<EPI_BIAS,128,128,2,2> 6 tiles (last 101 rows), dgrad N = 64:
         cg32_dgrad<256,64,1,2> 3 tiles (last 229), wgrad tiles 2 x 25 = 50, sp = 6, mps = 128, last split 101
  c3     128->256 3x3 on 10x7 (M = 210): fwd 128x128 2 x 2 tiles (last 82 rows), dgrad<128,128,2,2> 2 tiles,
         wgrad tiles 4 x 18 = 72, sp = 2, mps = 128, last split 82 rows
  c4     256->512 3x3 on 5x7 (M = 105): a single partial tile everywhere; wgrad tiles 8 x 36 = 288, sp = 1
``WRAPS`` -- tiles_m a little above the workgroups per column, so some workgroups take a second tile and
others do not, and the last tile is ragged:
  a512   64->512 3x3 on 5 x 75x90 (M = 33750): fold 0 cg32_fwd<EPI_BIAS,128,128,2,2> ntn = 4, gx = 256 against
         tiles_m = 264 (last 86 rows); fold 1 cg32_fwd<.,128,64,2,2,true> ntn = 8, gx = 128: every workgroup
         takes 2 tiles, eight take a third; wgrad tiles 8 x 9 = 72, sp = 7, mps = 4864, last split 4566 rows
  d512   512->64 3x3 on 5 x 75x90: fold 0 cg32_dgrad<128,128,2,2> ntn = 4, gx = 256 against 264; fold 1
         cg32_dgrad<128,64,2,2,true> ntn = 8, gx = 128 against 264
  b64    64->64 3x3 on 33 x 33x121 (M = 131769): cg32_fwd<EPI_BIAS,128,64,2,3> ntn = 1, gx = 1024 against
         tiles_m = 1030 (last 57 rows); fold 1 forward and dgrad (128x64 tiles) the same 1024 against 1030;
         wgrad tiles 9, sp = 56, mps = 2432, 55 splits used, the last of 441 rows
  e64    64->64 3x3 on 66 x 33x121 (M = 263538 > 262144), dgrad only, fold 0: cg32_dgrad<256,64,1,2>
         t256 = 1030 against 1024 workgroups (last tile 114 rows)
The largest case holds about 200 MB of tensors (e64: dy and dx of 67 MB each plus the reference chunks).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import cnn_lstm_helpers as ch
from deepfake_amd import _lib

pytestmark = pytest.mark.gpu

CONV_FLOOR = 2.0 ** -24
CHUNK_ROWS = 36000  # reference rows per chunk of whole images

# name: (N, H, W, Cin, Cout, k, stride, layout, launchers)
LAYERS = {
    "stem_cl": (3, 37, 51, 3, 64, 7, 2, "nhwc", "fw"),
    "stem_nchw": (3, 37, 51, 3, 64, 7, 2, "nchw", "fw"),
    "c2": (3, 19, 13, 64, 128, 5, 1, "nhwc", "fdw"),
    "c3": (3, 10, 7, 128, 256, 3, 1, "nhwc", "fdw"),
    "c4": (3, 5, 7, 256, 512, 3, 1, "nhwc", "fdw"),
}
WRAPS = {
    "a512": (5, 75, 90, 64, 512, 3, 1, "nhwc", "fw"),
    "d512": (5, 75, 90, 512, 64, 3, 1, "nhwc", "d"),
    "b64": (33, 33, 121, 64, 64, 3, 1, "nhwc", "fdw"),
    "e64": (66, 33, 121, 64, 64, 3, 1, "nhwc", "d"),
}


class _Err:
    """squared-error and squared-norm sums of (M, C) chunks against fp64: whole, per row, per column"""

    def __init__(self):
        self.rows_e, self.rows_n, self.col_e, self.col_n = [], [], 0.0, 0.0

    def add(self, got, ref):
        d = got.double() - ref
        self.rows_e.append((d * d).sum(1))
        self.rows_n.append((ref * ref).sum(1))
        self.col_e = self.col_e + (d * d).sum(0)
        self.col_n = self.col_n + (ref * ref).sum(0)

    def result(self):
        re, rn = torch.cat(self.rows_e), torch.cat(self.rows_n).sqrt()
        cn = self.col_n.sqrt()
        whole = float(re.sum().sqrt() / (cn.norm() + 1e-300))
        row = float((re.sqrt() / torch.maximum(rn, 0.05 * rn.median()).clamp_min(1e-300)).max())
        col = float((self.col_e.sqrt() / torch.maximum(cn, 0.05 * cn.median()).clamp_min(1e-300)).max())
        return whole, row, col


def _dw_err(got, ref):
    e = ch.bh.grad_errors({"w": got.cpu()}, {"w": ref.cpu()})["w"]
    return e[0], e[1]


def _judge(what, hip, anchor, names, bad):
    for n, e, a in zip(names, hip, anchor):
        q = e / max(a, CONV_FLOOR)
        print(f"  {what} {n}: err {e:.2e}, torch fp32 {a:.2e}, ratio {q:.2f} (K = {ch.K_CL})")
        if not e <= ch.K_CL * max(a, CONV_FLOOR):
            bad.append((what, n, e, a))


def _run(cuda, geom, fold):
    n, h, w, cin, cout, k, s, layout, which = geom
    lib, st = _lib.load(), _lib.stream_of(cuda)
    g = torch.Generator().manual_seed(1000 * cin + 10 * k + cout + h)
    p = k // 2
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    m_out = n * ho * wo
    wt = (torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5).to(cuda)
    bias = (0.5 * torch.randn(cout, generator=g)).to(cuda)
    x_nchw = torch.randn(n, cin, h, w, generator=g)
    if layout == "nhwc":
        x = x_nchw.permute(0, 2, 3, 1).contiguous().to(cuda)  # [n][y][x][c]
        xs = (ctypes.c_int64 * 4)(h * w * cin, w * cin, cin, 1)
        as_nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    else:
        x = x_nchw.contiguous().to(cuda)
        xs = (ctypes.c_int64 * 4)(cin * h * w, w, 1, h * w)  # element strides of (n, y, x, c)
        as_nchw = lambda t: t  # noqa: E731
    del x_nchw
    dy = torch.randn(n, ho, wo, cout, generator=g).to(cuda) if which != "f" else None
    wp = torch.empty(2 * wt.numel(), device=cuda)
    y = dx = dw = stats = None
    if "f" in which:
        rows = lib.dfd_rn_conv_stat_rows(n, ho, wo)
        stats = torch.empty(rows * 2 * cout, device=cuda)
        y = torch.empty(m_out, cout, device=cuda)
        _lib.check(lib.dfd_test_conv_fwd(st, x.data_ptr(), xs, n, h, w, cin, wt.data_ptr(), bias.data_ptr(), cout, k, k,
                                         s, p, fold, wp.data_ptr(), y.data_ptr(), stats.data_ptr()))
    if "d" in which:
        dx = torch.empty(n * h * w, cin, device=cuda)
        _lib.check(lib.dfd_test_conv_dgrad(st, dy.data_ptr(), n, h, w, cin, wt.data_ptr(), cout, k, k, s, p, fold,
                                           wp.data_ptr(), wp[wt.numel():].data_ptr(), dx.data_ptr()))
    if "w" in which:
        slab = torch.empty(max(8 * wt.numel(), 4 << 20), device=cuda)  # the model's slab rule (cl_layout)
        dw = torch.empty_like(wt)
        _lib.check(lib.dfd_test_conv_wgrad(st, x.data_ptr(), xs, n, h, w, cin, dy.data_ptr(), cout, k, k, s, p, fold,
                                           slab.data_ptr(), slab.numel(), dw.data_ptr()))
    torch.cuda.synchronize()

    # the reference and torch's own fp32, a few whole images at a time
    per = max(1, CHUNK_ROWS // max(h * w, ho * wo))
    ey, ey32, ex, ex32 = _Err(), _Err(), _Err(), _Err()
    w64, w32 = wt.double().requires_grad_("w" in which), wt.clone().requires_grad_("w" in which)
    y64 = torch.empty(m_out, cout, dtype=torch.float64, device=cuda) if "f" in which else None
    with torch.backends.cudnn.flags(enabled=False):
        for i0 in range(0, n, per):
            i1 = min(n, i0 + per)
            for dt, wr, e_y, e_x in ((torch.float64, w64, ey, ex), (torch.float32, w32, ey32, ex32)):
                xi = as_nchw(x[i0:i1]).to(dt).requires_grad_("d" in which)
                yr = F.conv2d(xi, wr, bias.to(dt), stride=s, padding=p)
                if which != "f":
                    yr.backward(dy[i0:i1].permute(0, 3, 1, 2).to(dt))
                yr = yr.detach().permute(0, 2, 3, 1).reshape(-1, cout)
                r0, r1 = i0 * ho * wo, i1 * ho * wo
                if dt == torch.float64:
                    if "f" in which:
                        y64[r0:r1] = yr
                        ey.add(y[r0:r1], yr)
                    if "d" in which:
                        ex.add(dx[i0 * h * w:i1 * h * w], xi.grad.permute(0, 2, 3, 1).reshape(-1, cin))
                        gx64 = xi.grad.permute(0, 2, 3, 1).reshape(-1, cin)
                else:
                    if "f" in which:
                        e_y.add(yr, y64[r0:r1])
                    if "d" in which:
                        e_x.add(xi.grad.permute(0, 2, 3, 1).reshape(-1, cin), gx64)
    bad = []
    tag = f"fold {fold}"
    if "f" in which:
        _judge(tag + " y", ey.result(), ey32.result(), ("tensor", "pixel row", "channel"), bad)
        # per 64-row tile: (sum, M2 about the tile's own mean) of y + bias -- the centred BatchNorm partials
        st2 = stats.view(rows, 2, cout).double()
        yt = F.pad(y64, (0, 0, 0, rows * 64 - m_out)).view(rows, 64, cout)
        nt = torch.full((rows,), 64.0, dtype=torch.float64, device=cuda)
        nt[-1] = m_out - 64 * (rows - 1)
        ts = yt.sum(1)
        valid = (torch.arange(64, device=cuda)[None, :] < nt[:, None])[:, :, None]
        m2 = (((yt - (ts / nt[:, None])[:, None, :]) ** 2) * valid).sum(1)
        torch.testing.assert_close(st2[:, 0], ts, rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(st2[:, 1], m2, rtol=1e-4, atol=1e-4)
        # the bias epilogue on its own: y - bias against the bias-free fp64 convolution of the first image
        with torch.backends.cudnn.flags(enabled=False):
            y0 = F.conv2d(as_nchw(x[:1]).double(), wt.double(), stride=s, padding=p)
        y0 = y0.permute(0, 2, 3, 1).reshape(-1, cout)
        torch.testing.assert_close(y[:ho * wo].double() - y0, bias.double().expand_as(y0), rtol=1e-5, atol=1e-5)
    if "d" in which:
        _judge(tag + " dx", ex.result(), ex32.result(), ("tensor", "pixel row", "channel"), bad)
    if "w" in which:
        _judge(tag + " dw", _dw_err(dw, w64.grad), _dw_err(w32.grad, w64.grad), ("tensor", "row"), bad)
    assert not bad, bad


@pytest.mark.parametrize("case", list(LAYERS))
def test_model_layer_geometries(cuda, case):
    """CNNLSTMHybrid's four convolutions (fold = 0, bias) at odd non-square maps"""
    _run(cuda, LAYERS[case], 0)


# the fold path has no 256 x 64 tile (e64); its 128 x 64 data-gradient loop wraps at b64 and d512
@pytest.mark.parametrize("case,fold", [(c, f) for f in (0, 1) for c in WRAPS if not (c == "e64" and f == 1)])
def test_persistent_grid_wraps(cuda, case, fold):
    """tiles_m just above the workgroups per tile column: the tile-advance code of every cg32 template"""
    _run(cuda, WRAPS[case], fold)
