"""Shared helpers for the whole-tensor CNN-LSTM gradient tests: the oracle side (``oracle.detector_cpu.
CNNLSTMHybridCPU`` in fp64 and fp32 on the CPU, cached per case and never modified by its users), the HIP
step, the inputs, and the bound.

The rule is the one of ``b0_helpers.py`` (``grad_errors`` / ``grad_bound_violations``): per tensor and per
dim-0 row, ``err_hip <= K_CL * max(err_torch_fp32, floor)``, both errors against the fp64 run.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import b0_helpers as bh
from deepfake_amd.weights import deterministic_init_
from oracle.detector_cpu import CNNLSTMHybridCPU

SEED = 31

# name: ((clips, frames per clip, H, W), hidden, layers, classes, input layout)
CASES = {
    "cl56": ((2, 3, 40, 56), 64, 2, 2, "channels_last"),
    "w100": ((1, 5, 36, 100), 72, 3, 2, "channels_last"),
    "nchw": ((3, 2, 50, 34), 64, 1, 3, "contiguous"),
    "t1": ((2, 1, 40, 56), 72, 2, 2, "channels_last"),
    "min": ((2, 2, 16, 24), 64, 2, 2, "channels_last"),
}

# With deterministic_init_ alone the temporal softmax is nearly uniform and attention.0.bias carries
# 1e-5 .. 1.4e-4 of the largest gradient norm -- not to be told from the structural zeros.  Every
# attention.* tensor of the init is therefore multiplied by ATT_SCALE, chosen on the CPU (fp64 oracle, seeds
# 31 .. 38 x scales 4 .. 64 scanned; above ~20 the softmax saturates and the gradients vanish again): with
# seed 31 and 14.0 every attention gradient is >= 1e-3 of the largest norm at every case (smallest: 1.07e-3,
# attention.2.weight in eval mode; 1.25e-3 at 1x5x36x100).  The other non-structural tensors are >= 1e-3 too
# except the BN shifts of the one-clip case 1x5x36x100 (cnn.9.bias 9.6e-4, cnn.5.bias 9.8e-4 of
# classifier.0.bias's norm): they do not depend on the attention (8.5e-4 .. 9.8e-4 at scales 1 .. 64, and
# below 1e-3 at 30 of the 31 seeds 39 .. 69), so their condition is MIN_SHARE_OTHER.
# tests/test_grad_checker.py::test_cl_conditions asserts both.
ATT_SCALE = 14.0
MIN_SHARE_ATT = 1e-3
MIN_SHARE_OTHER = 5e-4

# structurally zero gradients, by name: a conv bias that feeds a batch-statistics BN (training mode only),
# and the last attention bias (softmax over time is shift-invariant; both modes)
ZERO_TRAIN = frozenset(["cnn.0.bias", "cnn.4.bias", "cnn.8.bias", "cnn.12.bias", "attention.2.bias"])
ZERO_EVAL = frozenset(["attention.2.bias"])


def zeros(case, mode="train"):
    """the structurally zero gradients of a case, by name.  With one frame per clip (T = 1) the temporal
    softmax is the constant 1 and h_0 = 0, so every attention.* tensor and every lstm.weight_hh_l* is
    exactly zero as well (the fp64 oracle gives 0.0)."""
    z = set(ZERO_TRAIN if mode == "train" else ZERO_EVAL)
    (_, t, _, _), _, layers, _, _ = CASES[case]
    if t == 1:
        z |= {f"attention.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")}
        z |= {f"lstm.weight_hh_l{l}" for l in range(layers)}
    return frozenset(z)

# Floors: from the anchors themselves (torch fp32 vs fp64 on the CPU, seed 31, ATT_SCALE 14, the five
# training cases and the eval case; no HIP figure):
#   whole tensor: per-case median 5.4e-7 .. 4.4e-6, worst 9.5e-6 (lstm.weight_hh_l0 at 16x24),
#                 smallest 6.4e-10                                   -> CL_TENSOR_FLOOR = 5e-7
#   dim-0 rows:   per-case median 5.1e-6 .. 2.1e-5, worst 6.3e-4 (an lstm.weight_hh_l1 row at 16x24; every
#                 anchor at 16x24 is below 1e-3, so that case keeps the smallest accepted size)
#                                                                    -> CL_ROW_FLOOR = 5e-6
#   structural zeros: ||g_fp32|| = 1.1e-10 .. 2.9e-8 of the largest fp64 norm (exactly 0 for the T = 1
#                 attention / weight_hh tensors; fp64 itself <= 2.9e-17) -> CL_ZERO_FLOOR = 3e-8
#   running statistics after the step (relative L2 vs fp64): 3.4e-8 .. 4.7e-7, per-case median
#                 5.1e-8 .. 8.6e-8                                   -> CL_BUF_FLOOR = 2^-24 (6e-8)
# Pool condition (pool_agreement): fp32 and fp64 pick the same argmax in every window with a positive
# maximum; smallest relative top-2 gap in fp64: cl56 2.1e-6 (eval 1.1e-5), w100 1.8e-5, nchw 2.5e-5,
# t1 2.4e-6, min 4.7e-5 -- all above fp32's 6e-8 by a factor of 30 or more.
CL_TENSOR_FLOOR = 5e-7
CL_ROW_FLOOR = 5e-6
CL_ZERO_FLOOR = 3e-8
CL_BUF_FLOOR = 2.0 ** -24
# K_CL: the next power of two at or above twice the worst HIP ratio measured on the MI355X over every case
# of test_cnn_lstm_grad_full_gpu.py and test_conv_kernels_gpu.py; capped by the smallest planted-defect
# margin of tests/test_grad_checker.py (4000; CL_DEFECT_CAP = 2048 there).  Measured
# err_hip / max(err_torch_fp32, floor):
#   case    worst tensor                  worst dim-0 row               zeros   running statistics
#   cl56    1.08  cnn.1.weight            1.03  lstm.weight_hh_l1       0.12    1.01
#   w100    6.16  attention.0.weight      4.17  lstm.weight_ih_l0       0.11    1.01
#   nchw    8.09  lstm.weight_hh_l0       5.78  lstm.weight_hh_l0       0.12    1.88
#   t1      1.29  cnn.5.bias              1.31  lstm.weight_ih_l0       0.06    1.05
#   min     1.26  lstm.bias_ih_l1         1.16  cnn.12.weight           0.15    1.01
#   eval    1.64  classifier.3.weight     1.99  cnn.8.weight            0.005   (unchanged bit for bit)
#   conv launchers (test_conv_kernels_gpu.py): worst 4.51 (a pixel row of the 64->128 5x5 data gradient,
#   1.5e-6 against torch's 3.4e-7); every wrapped-grid case is below 1.
# The 8.09 is a whole-tensor error of 1.4e-5 where torch's is 1.7e-6: at nchw (three classes) every
# tensor downstream of the logits carries the same 1.4e-5 .. 1.5e-5 (cnn.13.bias, both LSTM biases,
# lstm.weight_ih_l0: 3.5 .. 3.8 x torch's 4e-6), one common factor from the loss gradient, and
# lstm.weight_hh_l0 happens to have the smallest torch error of them.  Twice 8.09 is 16.2: K_CL = 32.
K_CL = 32.0

_RUN = {}


def inputs(case):
    """(frames (B, T, 3, H, W) in the case's layout, labels)"""
    (b, t, h, w), _, _, nc, layout = CASES[case]
    x = bh.frames(SEED + 1, (b, t, 3, h, w))
    if layout == "channels_last":
        x = x.reshape(b * t, 3, h, w).contiguous(memory_format=torch.channels_last).view(b, t, 3, h, w)
    labels = torch.tensor([(i * 7 + 1) % nc for i in range(b)])
    return x, labels


def oracle_model(case):
    """the fp32 oracle module of a case with the step's initial weights (ATT_SCALE applied)"""
    _, hid, layers, nc, _ = CASES[case]
    m = CNNLSTMHybridCPU(3, hid, layers, nc, 0.0)
    deterministic_init_(m, seed=SEED)
    with torch.no_grad():
        for p in m.attention.parameters():
            p.mul_(ATT_SCALE)
    return m


POOLS = ("cnn.3", "cnn.7", "cnn.11")


def _run(case, mode, dtype, dy_hook=None):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    x, labels = inputs(case)
    m = oracle_model(case).to(dtype)
    m.train(mode == "train")
    pooled = {}
    hooks = [m.get_submodule(n).register_forward_hook(
        lambda _m, i, _o, n=n: pooled.__setitem__(n, i[0].detach())) for n in POOLS]
    if dy_hook is not None:
        name, fn = dy_hook
        hooks.append(m.get_submodule(name).register_full_backward_pre_hook(lambda _m, go: (fn(go[0]),)))
    before = {n: b.detach().clone() for n, b in m.named_buffers()}
    logits = m(x.to(dtype))
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    for h in hooks:
        h.remove()
    arg, gap = {}, 1.0
    for n, a in pooled.items():
        top, idx = F.max_pool2d(a, 3, 2, 1, return_indices=True)
        arg[n] = (idx, top > 0)
        if dtype == torch.float64:  # smallest relative gap between the two largest values of a window
            c = a.shape[1]
            win = F.unfold(a, 3, padding=1, stride=2).view(a.shape[0], c, 9, -1)  # zero padding: ReLU output
            t2 = win.topk(2, dim=2).values
            live = t2[:, :, 0] > 0
            gap = min(gap, float(((t2[:, :, 0] - t2[:, :, 1]) / t2[:, :, 0].clamp_min(1e-300))[live].min()))
    return dict(logits=logits.detach(), loss=float(loss.detach()),
                grads={n: p.grad.detach().clone() for n, p in m.named_parameters()},
                bufs={n: b.detach().clone() for n, b in m.named_buffers()}, bufs_before=before,
                argmax=arg, gap=gap)


def oracle(case, mode="train", dtype=torch.float32):
    """one cached oracle step (forward, CE, backward) of a case in ``mode`` ('train' / 'eval')"""
    key = (case, mode, dtype)
    if key not in _RUN:
        _RUN[key] = _run(case, mode, dtype)
    return _RUN[key]


def oracle64(case, mode="train"):
    return oracle(case, mode, torch.float64)


def oracle64_dy_hooked(case, module, fn):
    """the fp64 step with the output gradient of ``module`` replaced by fn(dY) (planted defects; not cached)"""
    return _run(case, "train", torch.float64, dy_hook=(module, fn))


def manual_lstm_grads(case, last_step_of=None):
    """The fp64 training step with the LSTM stack restated step by step from the module's own weights
    (gates i, f, g, o as nn.LSTM).  Returns {name: gradient}; with ``last_step_of`` = an lstm weight name,
    that weight's product at the last time step runs on a detached copy and the copy's gradient -- the
    last step's term of the sum over time -- is returned instead."""
    x, labels = inputs(case)
    m = oracle_model(case).double().train()
    (b, t, _, _), hid, layers, _, _ = CASES[case]
    p = dict(m.named_parameters())
    copy = p[last_step_of].detach().clone().requires_grad_(True) if last_step_of else None
    seq = m.cnn(x.double().reshape(b * t, 3, *x.shape[-2:])).view(b, t, 512)
    for l in range(layers):
        h = c = seq.new_zeros(b, hid)
        outs = []
        for s in range(t):
            w = {k: p[f"lstm.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
            for k in ("weight_ih", "weight_hh"):
                if s == t - 1 and last_step_of == f"lstm.{k}_l{l}":
                    w[k] = copy
            z = seq[:, s] @ w["weight_ih"].T + w["bias_ih"] + h @ w["weight_hh"].T + w["bias_hh"]
            i, f, g, o = z.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        seq = torch.stack(outs, dim=1)
    a = torch.softmax(m.attention(seq), dim=1)
    loss = F.cross_entropy(m.classifier((a * seq).sum(dim=1)), labels)
    loss.backward()
    if copy is not None:
        return copy.grad.detach()
    return {n: q.grad.detach() for n, q in p.items()}


def last_step_term(case, name):
    return manual_lstm_grads(case, last_step_of=name)


def pool_agreement(case, mode="train"):
    """(every max-pool argmax with a positive window maximum is the same in the fp32 and the fp64 oracle,
    smallest relative gap between the two largest values of such a window in fp64)"""
    a32, a64 = oracle(case, mode)["argmax"], oracle64(case, mode)["argmax"]
    same = all(bool((a32[n][0] == a64[n][0])[a64[n][1]].all()) and bool((a32[n][1] == a64[n][1]).all())
               for n in POOLS)
    return same, oracle64(case, mode)["gap"]


def anchor(case, mode="train"):
    key = (case, mode, "anchor")
    if key not in _RUN:
        _RUN[key] = bh.grad_errors(oracle(case, mode)["grads"], oracle64(case, mode)["grads"])
    return _RUN[key]


def grad_violations(got, case, mode="train", k=None, tag=""):
    """``got`` ({name: gradient}) by the anchored rule; the named structural zeros are bounded by
    ||g|| <= k * max(||g_torch_fp32||, CL_ZERO_FLOOR * scale), scale = the largest fp64 gradient norm.
    Returns (violations, worst tensor ratio, worst row ratio, worst structural-zero ratio)."""
    k = K_CL if k is None else k
    g64, g32 = oracle64(case, mode)["grads"], oracle(case, mode)["grads"]
    zs = zeros(case, mode)
    assert sorted(got) == sorted(g64) and zs <= set(g64)
    bad, wt, wc = bh.grad_bound_violations(got, g64, anchor(case, mode), k=k, tag=f"{case}/{mode}{tag}",
                                           tensor_floor=CL_TENSOR_FLOOR, channel_floor=CL_ROW_FLOOR, skip=zs)
    scale = max(float(r.norm()) for r in g64.values())
    wz = 0.0
    for n in sorted(zs):
        a = max(float(g32[n].double().norm()), CL_ZERO_FLOOR * scale)
        z = float(got[n].double().norm())
        wz = max(wz, z / a)
        if not z <= k * a:
            bad.append((n, "zero", z / scale, float(g32[n].double().norm()) / scale))
    print(f"{case}/{mode}{tag} structural zeros: worst ||g|| / max(||g_fp32||, floor) = {wz:.3f}")
    return bad, wt, wc, wz


def buf_violations(got, case, k=None, tag=""):
    """BN running statistics after the training step, anchored like the gradients: relative L2 error vs
    fp64 <= k * max(torch fp32's, CL_BUF_FLOOR); num_batches_tracked exactly."""
    k = K_CL if k is None else k
    b64, b32 = oracle64(case)["bufs"], oracle(case)["bufs"]
    bad, worst = [], 0.0
    assert sorted(got) == sorted(b64)
    for n, r in b64.items():
        if n.endswith("num_batches_tracked"):
            if int(got[n]) != int(r):
                bad.append((n, int(got[n]), int(r)))
            continue
        e, a = bh.rel_err(got[n], r), max(bh.rel_err(b32[n], r), CL_BUF_FLOOR)
        worst = max(worst, e / a)
        if not e <= k * a:
            bad.append((n, e, a))
    print(f"{case}{tag} running statistics: worst err / max(torch-fp32 err, floor) = {worst:.3f}")
    return bad, worst


def hip_step(case, cuda, mode="train"):
    """the same step on the HIP model: (logits, loss, {gradients}, {buffers after}), all on the CPU"""
    from deepfake_amd.cnn_lstm import CNNLSTMHybrid
    _, hid, layers, nc, _ = CASES[case]
    x, labels = inputs(case)
    m = CNNLSTMHybrid(3, hid, layers, nc, 0.0)
    m.load_state_dict(oracle_model(case).state_dict())
    m = m.to(cuda)
    m.train(mode == "train")
    logits = m(x.to(cuda))
    loss = F.cross_entropy(logits, labels.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    bufs = {n: b.detach().cpu() for n, b in m.named_buffers()}
    return logits.detach().cpu(), float(loss.detach()), grads, bufs
