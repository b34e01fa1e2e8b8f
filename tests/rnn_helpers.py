"""Shared helpers for the whole-tensor LogicRNNLSTM gradient tests: a plain-torch restatement of
``oracle.detector_cpu.LogicRNNLSTMCPU`` with an explicit sort permutation and explicit dropout keep-scale
tensors (fp32 and fp64 on the CPU, cached per case and never modified by its users), the NumPy restatement of
the library's counter-hash dropout, the HIP step, the inputs, and the bound.

The rule is the one of ``b0_helpers.py`` (``grad_errors`` / ``grad_bound_violations``): per tensor and per
dim-0 row, ``err_hip <= K_RNN * max(err_torch_fp32, floor)``, both errors against the fp64 run.  On top of it
every u-gate weight ``[H][in + H]`` is judged as two tensors, its x-column block ``[:, :in]`` (name + "[x]")
and its h-column block ``[:, in:]`` (name + "[h]"): the two halves come from different device buffers
(``rnn_scatter_kernel``) and at layer 0 the h half is much the smaller in norm, so a whole-tensor or whole-row
error would hide it.
"""
from __future__ import annotations

import re

import numpy as np
import torch
import torch.nn.functional as F

import b0_helpers as bh
import cnn_lstm_helpers as ch
from deepfake_amd.weights import deterministic_init_, hash_uniform
from oracle.detector_cpu import LogicRNNLSTMCPU

SEED = 41
DROP_SEED = 123  # torch.manual_seed before forward(); forward draws the kernel seed from the CPU generator

# name: (B, T, IN, H, L, lengths (original clip order) or None, dropout p)
CASES = {
    # distinct lengths, one of them 1; 4 and 5 exceed T = 3 and count as full clips (t < len holds for every t)
    "h128b5": (5, 3, 40, 128, 2, [3, 1, 2, 5, 4], 0.0),
    "h256b70": (70, 2, 64, 256, 3, [(i * 7) % 2 + 1 for i in range(70)], 0.3),        # ties: 35 of each
    "h384": (17, 4, 96, 384, 1, [(i * 5) % 4 + 1 for i in range(17)], 0.0),
    "h512": (33, 2, 128, 512, 2, None, 0.5),
    "h72": (3, 5, 48, 72, 2, [7, 2, 4], 0.3),                                         # 7 > T, un-clamped
    "t1": (4, 1, 32, 128, 2, [1, 3, 1, 2], 0.0),
    "nolen": (6, 3, 32, 128, 2, None, 0.0),
}
STEP_H = (128, 256, 384, 512)  # rnn_step_supported

U_GATES = ("and", "or", "forget", "input", "cell", "output")
_UW = re.compile(r"logic_cells\.(\d+)\.(and|or|forget|input|cell|output)_gate\.weight$")

# With deterministic_init_ alone the temporal softmax is nearly uniform and attention.0.bias -- sum_t ds_t = 0
# per clip, so only tanh's curvature keeps it from zero -- carries 4.5e-6 .. 1.1e-4 of the largest gradient
# norm, with a torch-fp32 error of up to 1.2e-4 of its own norm.  As in cnn_lstm_helpers.py every attention.*
# tensor of the init is multiplied by ATT_SCALE, scanned on the CPU over 1, 4, 8, 14, 24: from 4 up
# attention.0.bias is no longer the smallest gradient of any case, and 8 gives its smallest fp32 error
# (<= 5.5e-6; 14 and 24 saturate the softmax and the dim-0 row errors grow to 1.6e-5 and 1.0e-4).
ATT_SCALE = 8.0

# Floors start from the CNN-LSTM ones (CL_TENSOR_FLOOR 5e-7, CL_ROW_FLOOR 5e-6, CL_ZERO_FLOOR 3e-8) and are
# raised only as far as tests/test_grad_checker.py::test_rnn_fp32_oracle_passes_at_k1 needs: there the fp32
# oracle's gradients are judged at k = 1 against the anchor of a second fp32 run that sums in another order
# (``split_products``: x.Wx^T + h.Wh^T + b instead of cat(x, h).W^T + b), and the other way round, so a floor
# below fp32's own run-to-run spread fails.  Measured over the seven cases (torch fp32 against fp64 on the
# CPU, the larger of the two runs where they differ; no HIP figure):
#   whole tensor: 3.2e-7 (t1) .. 1.19e-6 (attention.2.weight at h384; attention.0.weight 1.17e-6)
#                                                            -> RNN_TENSOR_FLOOR = 2 x 1.5e-6  (CL: 5e-7)
#   attention.0.bias: 1.4e-6 .. 5.5e-6 (h256b70; the other run 1.7e-6): the cancelling sum above
#                                                            -> RNN_ATT_BIAS_FLOOR = 2 x 6e-6
#   dim-0 rows:   3.5e-6 .. 8.5e-6 (a logic_cells.0.and_gate.weight[x] row at t1; the other run 4.4e-6)
#                                                            -> RNN_ROW_FLOOR = 2 x 1e-5       (CL: 5e-6)
#   structural zeros: the fp32 oracle stays below 0.11 of CL_ZERO_FLOOR x scale: kept.
# The spread also depends on how many threads torch's CPU GEMMs use: with one thread the whole-tensor errors at
# h384 reach 1.65e-6 (the layer-0 biases).  Each floor is therefore twice the figure above, so that the k = 1
# test holds on a machine with another thread count.
RNN_TENSOR_FLOOR = 3e-6
RNN_ATT_BIAS_FLOOR = 1.2e-5
RNN_ROW_FLOOR = 2e-5
RNN_ZERO_FLOOR = ch.CL_ZERO_FLOOR
# K_RNN: the next power of two at least twice the worst HIP ratio measured on the MI355X over every case and
# both rnn_step settings of test_rnn_grad_full_gpu.py (the table is in that module's docstring): the worst is
# 1.18 (attention.0.weight at h384 on the sliced path, 3.5e-6 against torch's 1.1e-6 and the 3e-6 floor; the
# h-column blocks of layer 0 follow at 1.06), twice that is 2.4: K_RNN = 4.  No ratio comes near 16.  It is
# capped by the smallest planted-defect margin of tests/test_grad_checker.py (500; RNN_DEFECT_CAP = 256 there).
K_RNN = 4.0

_RUN = {}


def dims(case):
    b, t, i, h, l, _, p = CASES[case]
    return b, t, i, h, l, p


def inputs(case):
    """(x [B][T][IN] in clip order, lengths int64 [B] or None, targets [B][1] in SORTED row order)"""
    b, t, i, _, _, lens, _ = CASES[case]
    x = torch.from_numpy(hash_uniform(SEED + 1, f"rnn_x_{case}", b * t * i).reshape(b, t, i).copy())
    lengths = None if lens is None else torch.tensor(lens, dtype=torch.int64)
    target = torch.tensor([float((r * 7 + 1) % 3 != 0) for r in range(b)]).view(b, 1)
    return x, lengths, target


def cpu_perm(case):
    """the CPU's ``lengths.sort(0, descending=True)`` permutation (None without lengths)"""
    lengths = inputs(case)[1]
    return None if lengths is None else lengths.sort(0, descending=True)[1]


def oracle_model(case):
    _, _, i, h, l, _ = dims(case)
    m = LogicRNNLSTMCPU(i, h, l, 0.0)
    deterministic_init_(m, seed=SEED)
    with torch.no_grad():
        for q in m.attention.parameters():
            q.mul_(ATT_SCALE)
    return m


# ------------------------------------------------------------------ the counter-hash dropout, in NumPy
def drop_seed(s=DROP_SEED):
    """the seed ``LogicRNNLSTM.forward`` draws after ``torch.manual_seed(s)``"""
    torch.manual_seed(s)
    return int(torch.randint(0, 2**62, (1,)).item())


def keep_scale(seed, st, n, p):
    """keep-scale of elements 0 .. n-1 of stream ``st`` (``rnn_drop`` / ``drop_s``): float32 [n]"""
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (np.uint64(st) << np.uint64(56)) ^ (idx * np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    pf = np.float32(p)
    scale = np.float32(1) / (np.float32(1) - pf)
    return np.where(u >= pf, scale, np.float32(0)).astype(np.float32)


def masks(case, seed=None):
    """([one [B][T][H] keep-scale per inner layer], classifier [B][H]) of a case, indexed by SORTED row:
    inner layer l is stream l, element (b*T + t)*H + j; the classifier is stream 9, element b*H + j.
    All ones at p = 0."""
    b, t, _, h, l, p = dims(case)
    if p <= 0:
        return [torch.ones(b, t, h) for _ in range(l - 1)], torch.ones(b, h)
    seed = drop_seed() if seed is None else seed
    inner = [torch.from_numpy(keep_scale(seed, i, b * t * h, p).reshape(b, t, h)) for i in range(l - 1)]
    return inner, torch.from_numpy(keep_scale(seed, 9, b * h, p).reshape(b, h))


def keep_share_ok(mask, p):
    """(share of kept elements, within 4 binomial standard deviations of 1 - p and neither all nor none)"""
    n = mask.numel()
    kept = int((mask != 0).sum())
    share = kept / n
    ok = 0 < kept < n and abs(share - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5
    return share, ok


# ------------------------------------------------------------------ the oracle
class _MulBwd(torch.autograd.Function):
    """a * m whose backward multiplies by another mask (planted defects only)"""

    @staticmethod
    def forward(ctx, a, m, mb):
        ctx.mb = mb
        return a * m

    @staticmethod
    def backward(ctx, g):
        return g * ctx.mb, None, None


def _mul(a, m, mb=None):
    return a * m if mb is None else _MulBwd.apply(a, m, mb)


def _cell_split(cell, x, h, c):
    """``LogicCellCPU.forward`` with every u-gate product summed as x.Wx^T + h.Wh^T + b"""
    n = x.shape[1]

    def u(g):
        return x @ g.weight[:, :n].T + h @ g.weight[:, n:].T + g.bias
    a, o_ = torch.sigmoid(u(cell.and_gate)), torch.sigmoid(u(cell.or_gate))
    nn_ = torch.tanh(cell.not_gate(h))
    f, i, g = torch.sigmoid(u(cell.forget_gate)), torch.sigmoid(u(cell.input_gate)), torch.tanh(u(cell.cell_gate))
    c1 = f * c + i * g
    c2 = a * c1 + o_ * nn_
    return torch.sigmoid(u(cell.output_gate)) * torch.tanh(c2), c2


def oracle_forward(m, x, lengths, perm, inner, cls, inner_bwd=None, len_mask_bwd=True, split_products=False):
    """``LogicRNNLSTMCPU.forward`` (src/RNNModel.py:88-147) on module ``m``'s weights, with the sort permutation
    ``perm`` and the dropout keep-scale tensors handed in (``inner[l]`` [B][T][H] after layer l < L-1, ``cls``
    [B][H] after the classifier's ReLU; both indexed by sorted row).  ``inner_bwd`` / ``len_mask_bwd=False``
    replace the keep-scales / the length mask in the backward pass only (planted defects)."""
    b, t, _ = x.shape
    hid, layers = m.hidden_size, m.num_layers
    if lengths is not None:
        lengths = lengths[perm]
        x = x[perm]
    h = torch.zeros(b, hid, dtype=x.dtype)
    c = torch.zeros(b, hid, dtype=x.dtype)
    outs = []
    for s in range(t):
        hh, cc = h, c
        for i, cell in enumerate(m.logic_cells):
            xin = x[:, s] if i == 0 else hh
            hh, cc = _cell_split(cell, xin, hh, cc) if split_products else cell(xin, hh, cc)
            if i < layers - 1:
                hh = _mul(hh, inner[i][:, s], None if inner_bwd is None else inner_bwd[i][:, s])
        outs.append(hh)
        h, c = hh, cc
    o = torch.stack(outs, dim=1)
    if lengths is not None:
        mask = (torch.arange(t).expand(b, t) < lengths.unsqueeze(1)).to(x.dtype).unsqueeze(-1)
        o = _mul(o, mask, None if len_mask_bwd else torch.ones_like(mask))
    w = m.attention(o)
    ctx = (w * o).sum(dim=1)
    return torch.sigmoid(m.classifier[3](_mul(m.classifier[1](m.classifier[0](ctx)), cls)))


def run(case, dtype, perm, inner, cls, row_weight=None, **kw):
    """one oracle step (forward, BCE against the sorted-order targets, backward): y, loss, {gradients}.
    ``row_weight`` [B][1] weights the rows' loss terms (0 leaves a sorted row out of every gradient)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    x, lengths, target = inputs(case)
    m = oracle_model(case).to(dtype).train()
    y = oracle_forward(m, x.to(dtype), lengths, perm, [t.to(dtype) for t in inner], cls.to(dtype),
                       inner_bwd=None if kw.get("inner_bwd") is None else [t.to(dtype) for t in kw["inner_bwd"]],
                       len_mask_bwd=kw.get("len_mask_bwd", True), split_products=kw.get("split_products", False))
    loss = F.binary_cross_entropy(y, target.to(dtype), weight=None if row_weight is None else row_weight.to(dtype))
    loss.backward()
    return dict(y=y.detach(), loss=float(loss.detach()),
                grads={n: p.grad.detach().clone() for n, p in m.named_parameters()})


def oracle(case, perm, dtype=torch.float32):
    """the cached oracle step of a case under ``perm`` with the case's own dropout masks"""
    key = (case, dtype, None if perm is None else tuple(perm.tolist()))
    if key not in _RUN:
        _RUN[key] = run(case, dtype, perm, *masks(case))
    return _RUN[key]


def oracle64(case, perm):
    return oracle(case, perm, torch.float64)


# ------------------------------------------------------------------ the checker
def split(grads):
    """every u-gate weight gradient as its x-column block and its h-column block; everything else as is"""
    out = {}
    for n, g in grads.items():
        if _UW.match(n):
            nin = g.shape[1] - g.shape[0]
            out[n + "[x]"], out[n + "[h]"] = g[:, :nin], g[:, nin:]
        else:
            out[n] = g
    return out


def is_block(name):
    return name.endswith(("[x]", "[h]"))


def zeros(case):
    """the structurally zero (split) gradients of a case, by name.  attention.2.bias always: the softmax over
    time is shift invariant.  At T = 1 the softmax is the constant 1 and h = 0 enters layer 0: every
    attention.* tensor, layer 0's not_gate.weight and the h-column block of layer 0's six u-gates are zero
    (not_gate.bias is not: tanh(b_n) still feeds the cell); and c = 0 enters layer 0 too, so its forget gate,
    which only multiplies c, gets no gradient at all: forget_gate.bias and both forget_gate.weight blocks."""
    z = {"attention.2.bias"}
    if CASES[case][1] == 1:
        z |= {f"attention.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")}
        z |= {"logic_cells.0.not_gate.weight"}
        z |= {f"logic_cells.0.{g}_gate.weight[h]" for g in U_GATES}
        z |= {"logic_cells.0.forget_gate.weight[x]", "logic_cells.0.forget_gate.bias"}
    return frozenset(z)


def skipped_share(case):
    b, t, i, h, l, p = dims(case)
    return len(zeros(case)) / (l * 20 + 8)  # 7 weights (6 of them split in two) + 7 biases per layer, 8 head tensors


def anchor(case, perm):
    key = (case, "anchor", None if perm is None else tuple(perm.tolist()))
    if key not in _RUN:
        _RUN[key] = bh.grad_errors(split(oracle(case, perm)["grads"]), split(oracle64(case, perm)["grads"]))
    return _RUN[key]


def grad_violations(got, case, perm, k=None, tag="", anchor_=None):
    """``got`` ({parameter: gradient}) by the anchored rule, u-gate weights split into column blocks; the named
    structural zeros are bounded by ||g|| <= k * max(||g_torch_fp32||, RNN_ZERO_FLOOR * scale), scale = the
    largest fp64 gradient norm.  Returns (violations, worst tensor ratio, worst dim-0 row ratio, worst column
    block ratio (tensor or row), worst structural-zero ratio); the first two are over the unsplit tensors."""
    k = K_RNN if k is None else k
    g64, g32 = split(oracle64(case, perm)["grads"]), split(oracle(case, perm)["grads"])
    got = split(got)
    an = anchor(case, perm) if anchor_ is None else anchor_
    zs = zeros(case)
    assert sorted(got) == sorted(g64) and zs <= set(g64)
    bad, worst = [], []
    groups = ((" ", lambda n: not is_block(n) and n != "attention.0.bias", RNN_TENSOR_FLOOR),
              (" blocks", is_block, RNN_TENSOR_FLOOR), (" attention.0.bias", "attention.0.bias".__eq__, RNN_ATT_BIAS_FLOOR))
    for what, member, floor in groups:
        sub = {n: g for n, g in g64.items() if member(n)}
        b_, wt, wr = bh.grad_bound_violations(got, sub, an, k=k, tag=f"{case}{tag}{what}", tensor_floor=floor,
                                              channel_floor=RNN_ROW_FLOOR, skip=zs)
        bad += b_
        worst.append((wt, wr))
    scale = max(float(r.norm()) for r in g64.values())
    wz = 0.0
    for n in sorted(zs):
        a = max(float(g32[n].double().norm()), RNN_ZERO_FLOOR * scale)
        z = float(got[n].double().norm())
        wz = max(wz, z / a)
        if not z <= k * a:
            bad.append((n, "zero", z / scale, float(g32[n].double().norm()) / scale))
    print(f"{case}{tag} structural zeros: worst ||g|| / max(||g_fp32||, floor) = {wz:.3f}")
    return bad, max(worst[0][0], worst[2][0]), worst[0][1], max(worst[1]), wz


def old_rule_passes(got, ref):
    """what tests/test_rnn.py asked of a gradient before: norm within 1e-3 and the first 64 elements at
    rtol 1e-3 / atol 1e-6"""
    g, r = got.double().flatten(), ref.double().flatten()
    k = min(64, g.numel())
    return (abs(float(g.norm()) - float(r.norm())) <= 1e-3 * float(r.norm()) + 1e-7
            and bool(np.allclose(g[:k].numpy(), r[:k].numpy(), rtol=1e-3, atol=1e-6)))


# ------------------------------------------------------------------ the HIP side
def set_step_knob(on):
    """switch the per-cell launches (k_rnn_step.hip) on / off; returns the previous setting"""
    from deepfake_amd import _lib
    return _lib.load().dfd_set_tuning(b"rnn_step", 1 if on else 0)


def device_perm(case, cuda):
    """the permutation ``rnn.py`` itself takes: ``lengths.to(cuda).sort(0, descending=True)`` (tie order is
    the device's)"""
    lengths = inputs(case)[1]
    return None if lengths is None else lengths.to(cuda).sort(0, descending=True)[1].cpu()


def hip_model(case, cuda, p=None):
    from deepfake_amd.rnn import LogicRNNLSTM
    _, _, i, h, l, p_case = dims(case)
    m = LogicRNNLSTM(i, h, l, p_case if p is None else p)
    m.load_state_dict(oracle_model(case).state_dict())
    return m.to(cuda)


def hip_step(case, cuda):
    """the same step on the HIP model in train mode: (y, loss, {gradients}), all on the CPU"""
    x, lengths, target = inputs(case)
    m = hip_model(case, cuda).train()
    torch.manual_seed(DROP_SEED)
    y = m(x.to(cuda), None if lengths is None else lengths.to(cuda))
    loss = F.binary_cross_entropy(y, target.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), float(loss.detach()), {n: q.grad.detach().cpu() for n, q in m.named_parameters()}
