"""The kernels of ``csrc/k_vit.hip`` one by one, through the ``dfd_test_vit_*`` seam (thin calls of the
``launch_*`` functions ``csrc/vit.cpp`` uses), and the GCN head through ``dfd_gcn_head_forward/backward``.

Reference: plain PyTorch in fp64 of the same operands, rounded to the storage type first.
* fp32 storage: relative L2 error against fp64 <= K_KERNEL x max(torch's own fp32 error of the same operation,
  2^-24); K_KERNEL by the rule of ``vit_helpers.py`` (next power of two >= 2 x the worst ratio measured on the
  MI355X; figures in DESIGN.md).  Copies, casts and single additions are compared exactly.
* bf16 storage: element-wise within 2 bf16 ulps of the rounded reference plus 1e-3 x the reference RMS
  (``_close`` of ``test_vgemm_gpu.py``); fp32 outputs of bf16 operands (statistics, dgamma / dbeta, column
  sums) by the fp32 rule.

What the product path relies on in the pad columns [n, ld) of score rows (197 tokens in a 200-wide pitch),
read from the code: nothing.  ``bgemm_kernel`` stores only n < N and masks every operand read at k < K /
m < M element by element, so it neither writes nor reads them; ``softmax_fwd_kernel`` / ``softmax_bwd_kernel``
never read them and write them as exact zeros.  The tests fill input pads with NaN and output pads with a
sentinel and assert exactly that.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import b0_helpers as bh
import vit_helpers as vh
from deepfake_amd import _lib
from deepfake_amd.vit_gcn import _ptrs
from oracle.vit_cpu import SimpleGCNCPU

pytestmark = pytest.mark.gpu

DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16)}
K_KERNEL = 16.0  # measured worst 7.25: the mean of a single LayerNorm row (4.3e-7 against torch's 6e-8)
# the column sum clamped to ONE split adds 25,216 rows serially in fp32 where torch sums pairwise: measured 16.5 x
# torch's error there (2.9e-6 against 1.7e-7; every other column sum is below 2.2), so that case alone gets the
# next power of two above twice that.  vit.cpp's part_cap (6 Mi floats) never clamps the product's sums.
K_COLSUM_SERIAL = 64.0
FLOOR = 2.0 ** -24
SENT = 7.0
BIG_CAP = 2 * 1024 * 3072  # vit.cpp's part_cap


def _st(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _rand(gen, *shape, dtype=torch.float32, scale=1.0, cuda=None):
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(cuda)


def _close(got, ref, tag=""):
    scale = float(ref.float().pow(2).mean().sqrt())
    torch.testing.assert_close(got.float(), ref.bfloat16().float(), rtol=8e-3, atol=1e-3 * scale, msg=lambda m: f"{tag}: {m}")


def _anchored(got, ref64, t32, tag, k=K_KERNEL):
    """fp32 rule: rel. L2 of ``got`` vs fp64 within k x max(torch fp32's, 2^-24); prints the ratio"""
    e, a = bh.rel_err(got, ref64), max(bh.rel_err(t32, ref64), FLOOR)
    print(f"{tag}: err {e:.2e}, torch fp32 {a:.2e}, ratio {e / a:.2f} (K = {k})")
    assert e <= k * a, (tag, e, a)


def _judge(dtype, got, ref64, t32, tag):
    if dtype == "fp32":
        _anchored(got, ref64, t32, tag)
    else:
        _close(got, ref64, tag)


# ------------------------------------------------------------------ batched GEMM
def _tok(buf, nt, c0):
    """[2 * nt][W] token rows -> the [24][nt][64] per-(image, head) operand at column offset c0"""
    return buf.view(2, nt, -1)[:, :, c0:c0 + 768].reshape(2, nt, 12, 64).permute(0, 2, 1, 3).reshape(24, nt, 64)


# form: (ta, tb, A kind, B kind, C kind, alpha); kinds: ("tok", width, column offset) / ("score",)
BG_FORMS = {
    "qk": (0, 1, ("tok", 2304, 0), ("tok", 2304, 768), ("score",), 0.125),     # S = alpha q k^T
    "dp": (0, 1, ("tok", 768, 0), ("tok", 2304, 1536), ("score",), 1.0),       # dP = dO v^T
    "pv": (0, 0, ("score",), ("tok", 2304, 1536), ("tok", 768, 0), 1.0),       # O = P v
    "dq": (0, 0, ("score",), ("tok", 2304, 768), ("tok", 2304, 0), 0.125),     # dq = dS k
    "dk": (1, 0, ("score",), ("tok", 2304, 0), ("tok", 2304, 768), 1.0),       # dk = dS^T q
    "tt": (1, 1, ("score",), ("score",), ("score",), 0.125),                   # the fourth form: A^T B^T
}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nt", [197, 17, 1])
@pytest.mark.parametrize("form", list(BG_FORMS))
def test_bgemm(cuda, form, nt, dtype):
    code, tdt = DT[dtype]
    ta, tb, ka, kb, kc, alpha = BG_FORMS[form]
    ld = (nt + 7) // 8 * 8 + (0 if nt % 8 else 8) if nt > 8 else 8  # 197 -> 200, 17 -> 24, 1 -> 8
    gen = torch.Generator().manual_seed(nt + 7 * len(form))

    def make(kind, out):
        if kind[0] == "tok":
            buf = torch.full((2 * nt, kind[1]), SENT, dtype=tdt, device=cuda) if out else \
                _rand(gen, 2 * nt, kind[1], dtype=tdt, cuda=cuda)
            return buf, _i64(kind[1], 12, nt * kind[1], 64), kind[2]
        buf = torch.full((24 * nt, ld), SENT if out else float("nan"), dtype=tdt, device=cuda)
        if not out:
            buf[:, :nt] = _rand(gen, 24 * nt, nt, dtype=tdt, cuda=cuda)
        return buf, _i64(ld, 1, nt * ld, 0), 0

    def mats(kind, buf):
        return _tok(buf, nt, kind[2]) if kind[0] == "tok" else buf.view(24, nt, ld)[:, :, :nt]

    A, a4, ao = make(ka, False)
    B, b4, bo = make(kb, False)
    C, c4, co = make(kc, True)
    am, bm = mats(ka, A), mats(kb, B)
    opa = am.transpose(1, 2) if ta else am            # stored [k][m] -> [m][k]
    opb = bm.transpose(1, 2) if tb else bm            # stored [n][k] -> [k][n]
    M, K, N = opa.shape[1], opa.shape[2], opb.shape[2]
    assert opb.shape[1] == K
    es = A.element_size()
    _lib.check(_lib.load().dfd_test_vit_bgemm(_st(cuda), code, ta, tb, 24, M, N, K, alpha, A.data_ptr() + ao * es, a4,
                                              B.data_ptr() + bo * es, b4, C.data_ptr() + co * es, c4))
    torch.cuda.synchronize()
    ref = alpha * torch.bmm(opa.double(), opb.double())
    got = mats(kc, C)
    assert torch.isfinite(got.float()).all()  # the NaN pads of score operands are never read
    _judge(dtype, got, ref, alpha * torch.bmm(opa.float(), opb.float()), f"bgemm {form} nt={nt} {dtype}")
    untouched = C.clone()  # outside the M x N outputs (score pads, the other slices of qkv) the sentinel stays
    if kc[0] == "tok":
        untouched.view(2, nt, -1)[:, :, kc[2]:kc[2] + 768] = SENT
    else:
        untouched.view(24, nt, ld)[:, :, :nt] = SENT
    assert torch.equal(untouched, torch.full_like(C, SENT))


# ------------------------------------------------------------------ softmax
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n,ld,rows", [(197, 200, 1183), (17, 24, 207)])
def test_softmax(cuda, n, ld, rows, dtype):
    code, tdt = DT[dtype]
    lib = _lib.load()
    gen = torch.Generator().manual_seed(n)
    S = torch.full((rows, ld), float("nan"), dtype=tdt, device=cuda)
    s = torch.randn(rows, n, generator=gen) * 2.0
    s[5] += 50.0
    s[5, n - 2] += 80.0  # exp(130) overflows fp32 unless the row maximum is subtracted
    S[:, :n] = s.to(tdt).to(cuda)
    P = torch.full((rows, ld), SENT, dtype=tdt, device=cuda)
    _lib.check(lib.dfd_test_vit_softmax_fwd(_st(cuda), code, S.data_ptr(), P.data_ptr(), rows, n, ld))
    torch.cuda.synchronize()
    assert rows % 4 and torch.equal(P[:, n:], torch.zeros_like(P[:, n:]))
    s64 = S[:, :n].double()
    _judge(dtype, P[:, :n], torch.softmax(s64, 1), torch.softmax(S[:, :n].float(), 1), f"softmax_fwd n={n} {dtype}")
    assert float(P[5, n - 2]) > 0.99
    # backward: dS = scale * P * (dP - sum_j P dP), in place and out of place
    dP = torch.full((rows, ld), float("nan"), dtype=tdt, device=cuda)
    dP[:, :n] = _rand(gen, rows, n, dtype=tdt, cuda=cuda)
    dS = torch.full((rows, ld), SENT, dtype=tdt, device=cuda)
    _lib.check(lib.dfd_test_vit_softmax_bwd(_st(cuda), code, P.data_ptr(), dP.data_ptr(), dS.data_ptr(), rows, n, ld, 0.125))
    inpl = dP.clone()
    _lib.check(lib.dfd_test_vit_softmax_bwd(_st(cuda), code, P.data_ptr(), inpl.data_ptr(), inpl.data_ptr(), rows, n, ld, 0.125))
    torch.cuda.synchronize()
    assert torch.equal(dS, inpl) and torch.equal(dS[:, n:], torch.zeros_like(dS[:, n:]))

    def bwd(p, g):
        return 0.125 * p * (g - (p * g).sum(1, keepdim=True))
    _judge(dtype, dS[:, :n], bwd(P[:, :n].double(), dP[:, :n].double()), bwd(P[:, :n].float(), dP[:, :n].float()),
           f"softmax_bwd n={n} {dtype}")


# ------------------------------------------------------------------ LayerNorm
C = 768
LDS = 197 * C  # the final norm reads the CLS row of every image


def _ln_inputs(cuda, rows, ldx, tdt, seed, offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    X = torch.full((rows, ldx), float("nan"), dtype=tdt, device=cuda)
    X[:, :C] = (torch.randn(rows, C, generator=gen) * 1.5 + offset).to(tdt).to(cuda)
    g = (1.0 + 0.3 * torch.randn(C, generator=gen)).to(cuda)
    b = (0.2 * torch.randn(C, generator=gen)).to(cuda)
    return gen, X, g, b


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,strided,offset", [(1, 0, 0.0), (5, 0, 0.0), (197, 0, 0.0), (1, 1, 0.0), (5, 1, 0.0),
                                                  (197, 1, 0.0), (197, 0, 1500.0)])
def test_ln_fwd(cuda, rows, strided, offset, dtype):
    """offset 1500: mean ~ 1e3 x std, which a one-pass E[x^2] - mean^2 variance would lose in fp32"""
    code, tdt = DT[dtype]
    ldx = LDS if strided else C
    _, X, g, b = _ln_inputs(cuda, rows, ldx, tdt, rows + strided, offset)
    out_f32 = 1 if (strided and dtype == "bf16") else 0  # the final norm writes fp32 features
    Y = torch.full((rows, C), SENT, dtype=torch.float32 if out_f32 else tdt, device=cuda)
    mean, rstd = torch.empty(rows, device=cuda), torch.empty(rows, device=cuda)
    _lib.check(_lib.load().dfd_test_vit_ln_fwd(_st(cuda), code, out_f32, X.data_ptr(), ldx, g.data_ptr(), b.data_ptr(),
                                               Y.data_ptr(), C, mean.data_ptr(), rstd.data_ptr(), rows, C, 1e-6))
    torch.cuda.synchronize()
    x = X[:, :C]
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)
    t32 = F.layer_norm(x.float(), (C,), g, b, 1e-6)
    tag = f"ln_fwd rows={rows} strided={strided} offset={offset} {dtype}"
    _judge("fp32" if out_f32 else dtype, Y, ref, t32, tag)
    x64 = x.double()
    _anchored(mean, x64.mean(1), x.float().mean(1), tag + " mean")
    _anchored(rstd, (x64.var(1, unbiased=False) + 1e-6).rsqrt(), (x.float().var(1, unbiased=False) + 1e-6).rsqrt(),
              tag + " rstd")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,dres,strided,cap", [(1, 0, 0, BIG_CAP), (1, 1, 0, BIG_CAP), (17, 0, 0, BIG_CAP),
                                                   (17, 1, 0, BIG_CAP), (197, 0, 0, BIG_CAP), (197, 1, 0, BIG_CAP),
                                                   (1182, 0, 0, BIG_CAP), (1182, 1, 0, BIG_CAP),
                                                   (197, 1, 0, 2 * C), (197, 1, 0, 6 * C + 5),  # 1 and 3 workgroups
                                                   (1, 0, 1, BIG_CAP), (17, 0, 1, BIG_CAP)])        # the final norm's form
def test_ln_bwd(cuda, rows, dres, strided, cap, dtype):
    """cap 2C: one workgroup takes all 197 rows; 6C + 5: three of rpb = 66 (the last one 65 rows); the
    default: cdiv(rows, 16) workgroups (13 at 197 rows, 74 at 1182).  strided: X / dX rows 197 x 768 apart and
    dY in fp32 (the final norm over the CLS rows).  No caller passes accumulate, so it is not exercised."""
    code, tdt = DT[dtype]
    lib = _lib.load()
    ldx = LDS if strided else C
    gen, X, g, _ = _ln_inputs(cuda, rows, ldx, tdt, 3 * rows + dres + strided)
    dy_f32 = 1 if (strided and dtype == "bf16") else 0
    ddt = torch.float32 if dy_f32 else tdt
    dY = _rand(gen, rows, C, dtype=ddt, cuda=cuda)
    R = None
    if dres:
        R = torch.full((rows, ldx), float("nan"), dtype=tdt, device=cuda)
        R[:, :C] = _rand(gen, rows, C, dtype=tdt, cuda=cuda)
    x64 = X[:, :C].double()
    mean = x64.mean(1).float()
    rstd = (x64.var(1, unbiased=False) + 1e-6).rsqrt().float()
    outs = []
    for adjacent in (True, False):
        dX = torch.full((rows, ldx), SENT, dtype=tdt, device=cuda)
        part = torch.empty(cap, device=cuda)
        gb = torch.full((2 * C,), SENT, device=cuda)
        dg, db = (gb[:C], gb[C:]) if adjacent else (torch.full((C,), SENT, device=cuda), torch.full((C,), SENT, device=cuda))
        _lib.check(lib.dfd_test_vit_ln_bwd(_st(cuda), code, dy_f32, X.data_ptr(), ldx, dY.data_ptr(), C, g.data_ptr(),
                                           mean.data_ptr(), rstd.data_ptr(), R.data_ptr() if dres else None,
                                           dX.data_ptr(), rows, C, part.data_ptr(), cap, dg.data_ptr(), db.data_ptr(), 0))
        torch.cuda.synchronize()
        outs.append((dX, dg.clone(), db.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    dX, dg, db = outs[0]
    if strided:
        assert torch.equal(dX[:, C:], torch.full_like(dX[:, C:], SENT))  # only the CLS rows are written

    def ref(dt):
        x = X[:, :C].to(dt).requires_grad_(True)
        gg = g.to(dt).requires_grad_(True)
        bb = torch.zeros(C, dtype=dt, device=cuda, requires_grad=True)
        F.layer_norm(x, (C,), gg, bb, 1e-6).backward(dY.to(dt))
        return x.grad + (R[:, :C].to(dt) if dres else 0), gg.grad, bb.grad
    r64, r32 = ref(torch.float64), ref(torch.float32)
    tag = f"ln_bwd rows={rows} dres={dres} strided={strided} cap={cap} {dtype}"
    _judge(dtype, dX[:, :C], r64[0], r32[0], tag + " dX")
    _anchored(dg, r64[1], r32[1], tag + " dgamma")
    _anchored(db, r64[2], r32[2], tag + " dbeta")


# ------------------------------------------------------------------ patch gather, tokens
def _images(cuda, b, n, layout, seed):
    x = bh.frames(seed, (b, n, 3, 224, 224)).to(cuda)
    if layout == "channels_last":
        x = x.reshape(b * n, 3, 224, 224).contiguous(memory_format=torch.channels_last).view(b, n, 3, 224, 224)
    elif layout == "sliced":  # a slice of a larger batch: batch, node and channel strides all differ
        big = torch.full((b + 1, n + 1, 4, 224, 224), float("nan"), device=cuda)
        big[1:, 1:, :3] = x
        x = big[1:, 1:, :3]
    plain = (n * 3 * 224 * 224, 3 * 224 * 224, 224 * 224, 224, 1)
    assert (tuple(x.stride()) == plain) == (layout == "contiguous")
    return x


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "sliced"])
@pytest.mark.parametrize("b,n", [(1, 1), (2, 3), (1, 9)])
def test_patch_gather(cuda, b, n, layout, dtype):
    code, tdt = DT[dtype]
    x = _images(cuda, b, n, layout, 50 + n)
    A = torch.full((b * n * 196, C), SENT, dtype=tdt, device=cuda)
    _lib.check(_lib.load().dfd_test_vit_patch_gather(_st(cuda), code, x.data_ptr(), _i64(*x.stride()), n, 224, 224,
                                                     b * n, A.data_ptr()))
    torch.cuda.synchronize()
    xc = x.reshape(b * n, 3, 224, 224)
    ref = F.unfold(xc, 16, stride=16).transpose(1, 2).reshape(-1, C)  # k = c * 256 + ky * 16 + kx
    assert torch.equal(A, ref.to(tdt))  # fp32: a copy; bf16: the round-to-nearest-even of the source
    if dtype == "fp32":  # the ordering is Conv2d.weight.flatten(1)'s
        w = _rand(torch.Generator().manual_seed(3), 32, 3, 16, 16, cuda=cuda).double()
        with torch.backends.cudnn.flags(enabled=False):
            y = F.conv2d(xc.double(), w, stride=16).flatten(2).transpose(1, 2).reshape(-1, 32)
        assert bh.rel_err(A.double() @ w.flatten(1).T, y) <= 1e-12


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("images", [1, 7, 8, 9, 17])
def test_tokens(cuda, images, dtype):
    code, tdt = DT[dtype]
    lib = _lib.load()
    gen = torch.Generator().manual_seed(images)
    PE = _rand(gen, images * 196, C, dtype=tdt, cuda=cuda)
    cls, pos = _rand(gen, C, cuda=cuda), _rand(gen, 197, C, cuda=cuda)
    X0 = torch.full((images, 197, C), SENT, dtype=tdt, device=cuda)
    _lib.check(lib.dfd_test_vit_tokens_fwd(_st(cuda), code, PE.data_ptr(), cls.data_ptr(), pos.data_ptr(), images, 197, C,
                                           X0.data_ptr()))
    torch.cuda.synchronize()
    ref = torch.cat([cls.expand(images, 1, C), PE.float().view(images, 196, C)], 1) + pos
    assert torch.equal(X0, ref.to(tdt))  # one fp32 addition, rounded once
    dX0 = _rand(gen, images, 197, C, dtype=tdt, cuda=cuda)
    dPE = torch.full((images * 196, C), SENT, dtype=tdt, device=cuda)
    dpos, dcls = torch.full((197, C), SENT, device=cuda), torch.full((C,), SENT, device=cuda)
    _lib.check(lib.dfd_test_vit_tokens_bwd(_st(cuda), code, dX0.data_ptr(), images, 197, C, dPE.data_ptr(), dpos.data_ptr(),
                                           dcls.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(dPE.view(images, 196, C), dX0[:, 1:])  # a pure copy
    assert torch.equal(dcls, dpos[0])
    _anchored(dpos, dX0.double().sum(0), dX0.float().sum(0), f"tokens_bwd images={images} {dtype} dpos")


# ------------------------------------------------------------------ weight cast, column sum, GELU passes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shapes,both", [([(2304, 768), (768, 768), (3072, 768), (768, 3072)], True),
                                         ([(768, 768)], False), ([(40, 72)], True), ([(40, 72), (768, 768)], True)])
def test_wcast(cuda, shapes, both, dtype):
    """one block's four segments in one launch (bf16: the 64 x 64 kernel), the patch embedding's single
    untransposed segment, and a [40, 72] segment: ragged in both dims of the 32 x 32 tiles, alone and next to
    a larger segment (the grid then spans the larger one's tiles)"""
    code, tdt = DT[dtype]
    gen = torch.Generator().manual_seed(len(shapes))
    src = [_rand(gen, r, c, cuda=cuda) for r, c in shapes]
    dst = [torch.full((r, c), SENT, dtype=tdt, device=cuda) for r, c in shapes]
    dst_t = [torch.full((c, r), SENT, dtype=tdt, device=cuda) for r, c in shapes] if both else [None] * len(shapes)
    none = (ctypes.c_void_p * len(shapes))()
    rows = (ctypes.c_int * len(shapes))(*[r for r, _ in shapes])
    cols = (ctypes.c_int * len(shapes))(*[c for _, c in shapes])
    _lib.check(_lib.load().dfd_test_vit_wcast(_st(cuda), code, len(shapes), _ptrs(src), _ptrs(dst),
                                              _ptrs(dst_t) if both else none, rows, cols))
    torch.cuda.synchronize()
    for s, d, t in zip(src, dst, dst_t):
        assert torch.equal(d, s.to(tdt))
        if both:
            assert torch.equal(t, s.to(tdt).t())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [768, 2304])
@pytest.mark.parametrize("M,cap", [(1, BIG_CAP), (63, BIG_CAP), (197, BIG_CAP), (25216, BIG_CAP), (197, 0), (25216, 0)])
def test_colsum(cuda, M, N, cap, dtype):
    """cap 0 -> part_cap = N: one split sums every row; the default: min(cdiv(M, 64), 256) splits"""
    code, tdt = DT[dtype]
    cap = cap or N
    X = _rand(torch.Generator().manual_seed(M + N), M, N, dtype=tdt, cuda=cuda)
    part, out = torch.empty(min(cap, 256 * N), device=cuda), torch.full((N,), SENT, device=cuda)
    _lib.check(_lib.load().dfd_test_vit_colsum(_st(cuda), code, X.data_ptr(), M, N, part.data_ptr(), cap, out.data_ptr(), 0))
    torch.cuda.synchronize()
    _anchored(out, X.double().sum(0), X.float().sum(0), f"colsum M={M} N={N} cap={cap} {dtype}",
              K_COLSUM_SERIAL if (cap == N and M > 64) else K_KERNEL)


def test_gelu_passes(cuda):
    """launch_gelu's contract: n % 8 == 0 (8 bf16 per lane), anything else is refused; n = 8 x 1001 leaves a
    partial last workgroup"""
    lib = _lib.load()
    n = 8 * 1001
    gen = torch.Generator().manual_seed(9)
    z = _rand(gen, n, dtype=torch.bfloat16, scale=2.0, cuda=cuda)
    Z, G = z.clone(), torch.full((n,), SENT, dtype=torch.bfloat16, device=cuda)
    _lib.check(lib.dfd_test_vit_gelu(_st(cuda), Z.data_ptr(), G.data_ptr(), n, 0))
    torch.cuda.synchronize()
    z64 = z.double()
    cdf = 0.5 * (1.0 + torch.erf(z64 / 2.0 ** 0.5))
    _close(G, z64 * cdf, "gelu")
    _close(Z, cdf + z64 * torch.exp(-0.5 * z64 * z64) / (2.0 * torch.pi) ** 0.5, "gelu'")
    d, dz = _rand(gen, n, dtype=torch.bfloat16, cuda=cuda), _rand(gen, n, dtype=torch.bfloat16, cuda=cuda)
    out = dz.clone()
    _lib.check(lib.dfd_test_vit_gelu(_st(cuda), d.data_ptr(), out.data_ptr(), n, 1))
    torch.cuda.synchronize()
    assert torch.equal(out, (dz.float() * d.float()).bfloat16())  # an exact fp32 product, rounded once
    with pytest.raises(_lib.DFDError):
        _lib.check(lib.dfd_test_vit_gelu(_st(cuda), Z.data_ptr(), G.data_ptr(), n - 3, 0))


# ------------------------------------------------------------------ the GCN head on its own
HB, HN, HDV, HHID, HOUT, HC = 3, 5, 768, 200, 72, 3
HDIMS = (HB, HN, HDV, HHID, HOUT, HC)


def _head_setup(cuda):
    gen = torch.Generator().manual_seed(77)
    gcn = SimpleGCNCPU(HDV, HHID, HOUT, 0.0)
    cls = torch.nn.Sequential(torch.nn.Linear(HOUT, 64), torch.nn.ReLU(), torch.nn.Dropout(0.0), torch.nn.Linear(64, HC))
    params = [p.detach().to(cuda) for p in list(gcn.parameters()) + list(cls.parameters())]
    feats = _rand(gen, HB * HN, HDV, cuda=cuda)
    a = torch.rand(HB, HN, HN, generator=gen) + 0.1
    a = (a / a.sum(2, keepdim=True)).to(cuda)
    assert not torch.allclose(a, a.transpose(1, 2))
    dlogits = _rand(gen, HB, HC, cuda=cuda)
    return params, feats, a, dlogits


def _head_hip(cuda, params, feats, a, dlogits, p, seed):
    lib = _lib.load()
    work = torch.zeros(int(lib.dfd_gcn_head_work_floats(*HDIMS)), device=cuda)
    scratch = torch.zeros(int(lib.dfd_gcn_head_scratch_floats(*HDIMS)), device=cuda)
    logits = torch.empty(HB, HC, device=cuda)
    _lib.check(lib.dfd_gcn_head_forward(_st(cuda), *HDIMS, feats.data_ptr(), a.data_ptr(), _ptrs(params), work.data_ptr(),
                                        1, seed, p, logits.data_ptr()))
    grads = [torch.full_like(q, SENT) for q in params]
    dfeats = torch.full_like(feats, SENT)
    _lib.check(lib.dfd_gcn_head_backward(_st(cuda), *HDIMS, a.data_ptr(), _ptrs(params), work.data_ptr(), scratch.data_ptr(),
                                         1, seed, p, dlogits.data_ptr(), _ptrs(grads), dfeats.data_ptr()))
    torch.cuda.synchronize()
    return logits, grads, dfeats, work


def _head_ref(dt, params, feats, a, dlogits, m1=None, m2=None):
    """fp64 / fp32 head with given dropout masks (already scaled by 1 / (1 - p)); (logits, grads, dfeats)"""
    ps = [q.to(dt).requires_grad_(True) for q in params]
    f = feats.to(dt).requires_grad_(True)
    h = torch.bmm(a.to(dt), f.view(HB, HN, HDV)).view(HB * HN, HDV)
    d1 = F.relu(h @ ps[0].T + ps[1]) * (1 if m1 is None else m1.to(dt))
    y2 = F.relu(d1 @ ps[2].T + ps[3])
    c1 = F.relu(y2.view(HB, HN, HOUT).mean(1) @ ps[4].T + ps[5]) * (1 if m2 is None else m2.to(dt))
    logits = c1 @ ps[6].T + ps[7]
    logits.backward(dlogits.to(dt))
    return logits.detach(), [q.grad for q in ps], f.grad


def _head_judge(got, params, feats, a, dlogits, m1, m2, tag):
    names = ["gcn.fc1.weight", "gcn.fc1.bias", "gcn.fc2.weight", "gcn.fc2.bias", "classifier.0.weight",
             "classifier.0.bias", "classifier.3.weight", "classifier.3.bias", "dfeats", "logits"]
    r64 = _head_ref(torch.float64, params, feats, a, dlogits, m1, m2)
    r32 = _head_ref(torch.float32, params, feats, a, dlogits, m1, m2)
    flat = lambda r: dict(zip(names, [g.cpu() for g in r[1]] + [r[2].cpu(), r[0].cpu()]))  # noqa: E731
    g64 = flat(r64)
    an = bh.grad_errors(flat(r32), g64, columns=True)
    bad, wt, wr, wc = bh.grad_bound_violations(flat(got), g64, an, k=vh.K_VIT, tag=tag, tensor_floor=vh.VIT_TENSOR_FLOOR,
                                               channel_floor=vh.VIT_ROW_FLOOR, skip=frozenset(),
                                               column_floor=vh.VIT_COL_FLOOR)
    print(f"{tag}: worst ratios tensor {wt:.2f}, row {wr:.2f}, column {wc:.2f} (K_VIT = {vh.K_VIT})")
    assert not bad, bad


def test_gcn_head_p0(cuda):
    params, feats, a, dlogits = _head_setup(cuda)
    logits, grads, dfeats, _ = _head_hip(cuda, params, feats, a, dlogits, 0.0, 0)
    _head_judge((logits, grads, dfeats), params, feats, a, dlogits, None, None, "gcn head p=0")


def test_gcn_head_dropout_mask_shared_by_forward_and_backward(cuda):
    """p = 0.3: the mask is the library's counter hash, which torch cannot reproduce, so it is read back from the
    forward's work buffer (offsets from dfd_test_gcn_head_offsets: Y1 = relu output, D1 = after dropout; C1 /
    Dc for classifier[2]) and the backward is compared with the fp64 head built with that mask."""
    p, seed = 0.3, 1234567
    lib = _lib.load()
    params, feats, a, dlogits = _head_setup(cuda)
    logits, grads, dfeats, work = _head_hip(cuda, params, feats, a, dlogits, p, seed)
    off = (ctypes.c_int64 * 7)()
    _lib.check(lib.dfd_test_gcn_head_offsets(*HDIMS, off))
    bn = HB * HN
    y1, d1 = work[off[1]:off[1] + bn * HHID].view(bn, HHID), work[off[2]:off[2] + bn * HHID].view(bn, HHID)
    c1, dc = work[off[5]:off[5] + HB * 64].view(HB, 64), work[off[6]:off[6] + HB * 64].view(HB, 64)
    masks = []
    for y, d, what in ((y1, d1, "gcn.dropout"), (c1, dc, "classifier[2]")):
        live = y > 0
        assert bool((y >= 0).all()) and int(live.sum()) > 0.2 * y.numel()
        keep = live & (d != 0)
        assert torch.equal(d[keep], (y * (1.0 / (1.0 - p)))[keep]) or torch.allclose(d[keep], y[keep] / (1.0 - p), rtol=2e-7, atol=0)
        assert bool((d[~keep] == 0).all())
        n, share = int(live.sum()), float(keep.sum()) / float(live.sum())
        sd = (p * (1 - p) / n) ** 0.5
        print(f"{what}: kept {share:.4f} of {n} live elements (1 - p = {1 - p}, 4 sd = {4 * sd:.4f})")
        assert abs(share - (1 - p)) <= 4 * sd
        masks.append(keep.float() / (1.0 - p))
    # dead (relu = 0) elements carry no gradient either way, so their mask value does not matter
    l2, g2, df2, w2 = _head_hip(cuda, params, feats, a, dlogits, p, seed)
    assert torch.equal(l2, logits) and torch.equal(w2, work) and torch.equal(df2, dfeats)
    assert all(torch.equal(x, y) for x, y in zip(g2, grads))
    l3 = _head_hip(cuda, params, feats, a, dlogits, p, seed + 1)[0]
    assert not torch.equal(l3, logits)
    _head_judge((logits, grads, dfeats), params, feats, a, dlogits, masks[0], masks[1], "gcn head p=0.3")
