"""Shared helpers for the whole-tensor DeepfakeModel (ViT-B/16 + SimpleGCN) gradient tests: the oracle side
(``oracle.vit_cpu.DeepfakeModelCPU`` in fp64, fp32 and under torch's bf16 autocast, as plain PyTorch on the
device it is given -- the GPU with MIOpen off in the GPU tests, the CPU in ``test_grad_checker.py`` --
cached per case and never modified by its users), the HIP step, the inputs, and the bound.

The rule is the one of ``b0_helpers.py`` (``grad_errors`` / ``grad_bound_violations``) with the column check
switched on: per tensor, per dim-0 row and, for 2-D tensors, per dim-1 column,
``err_hip <= K x max(err_torch, floor)``, both errors against the fp64 run of the same step.  ``err_torch``
is torch's own fp32 step for the fp32 path (``K_VIT``) and torch's bf16 autocast step for the bf16 path
(``K_VIT_BF16``).  ``attn.qkv.weight`` / ``.bias`` are judged as their q, k and v slices (``split``): a
swapped or stale slice then shows as a whole-tensor error of that slice.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import b0_helpers as bh
from deepfake_amd.weights import deterministic_init_
from oracle.vit_cpu import DeepfakeModelCPU

SEED = 41
E = 768

# name: clips B, nodes N, depth, classes, gcn_hid, gcn_out, adjacency, dtypes
CASES = {
    "A": dict(B=2, N=3, depth=12, classes=2, hid=256, out=128, adj="sym", dtypes=("fp32", "bf16")),
    "B": dict(B=1, N=1, depth=1, classes=2, hid=256, out=128, adj="sym", dtypes=("fp32", "bf16")),
    "C": dict(B=3, N=3, depth=3, classes=3, hid=200, out=72, adj="asym", dtypes=("fp32", "bf16")),
    "D": dict(B=2, N=37, depth=1, classes=2, hid=256, out=128, adj="sym", dtypes=("bf16",)),
    # the CPU self-test of the checker (test_grad_checker.py): depth 3 on 2 x 2 images
    "P": dict(B=2, N=2, depth=3, classes=2, hid=256, out=128, adj="asym", dtypes=()),
    "Psym": dict(B=2, N=2, depth=3, classes=2, hid=256, out=128, adj="sym", dtypes=()),
}

# Structural zeros, by name (after ``split``): the key slice of every attn.qkv.bias.  softmax over the keys
# is invariant to a constant added to every key's score, and a key bias adds q_i . b_k to every score of
# query i, so its gradient is exactly zero (the fp64 oracle gives <= 1e-17 of the largest norm).  No other
# gradient of the model is structurally zero at head dropout 0 (test_grad_checker.py::test_vit_conditions
# asserts both).


def zeros(case):
    return frozenset(f"vit.vit.blocks.{l}.attn.qkv.bias[k]" for l in range(CASES[case]["depth"]))


# ---- floors and K ("Whole-tensor ViT + GCN gradient check").
# Floors come from the anchors alone (torch against fp64, plain PyTorch on the MI355X, cases A - D, seed 41, the
# init of ``oracle_model``; no HIP figure): the smallest per-case median anchor, rounded down, as CL_*_FLOOR.
#   torch fp32 vs fp64, per-case median (max):   tensor 5.4e-7 .. 2.9e-6 (4.7e-6)   -> VIT_TENSOR_FLOOR = 5e-7
#                                                dim-0 row 3.9e-6 .. 2.3e-5 (2.3e-4) -> VIT_ROW_FLOOR = 3.8e-6
#                                                dim-1 column 9.6e-6 .. 7.4e-5 (2.4e-4) -> VIT_COL_FLOOR = 9e-6
#   key-bias slices: ||g_fp32|| = 3.8e-10 .. 7.8e-9 of the largest fp64 norm        -> VIT_ZERO_FLOOR = 8e-9
#   torch bf16 autocast vs fp64, per-case median (max): tensor 1.2e-2 .. 1.4e-1 (1.6e-1) -> VIT16_TENSOR_FLOOR = 1e-2
#                                                dim-0 row 1.0e-1 .. 2.0 (10.7)      -> VIT16_ROW_FLOOR = 1e-1
#                                                dim-1 column 8.5e-2 .. 4.5e-1 (1.5) -> VIT16_COL_FLOOR = 8e-2
#   key-bias slices under autocast: 1.5e-6 .. 5.1e-5 of the largest fp64 norm       -> VIT16_ZERO_FLOOR = 5e-5
# torch's own bf16 autocast step of this model is 1 % .. 16 % off per tensor and 10 % .. 1000 % off on single
# rows: with deterministic_init_ the bf16 step is that ill-conditioned, so the bf16 rule can see only gross
# defects (a swapped slice, a stale buffer); the planted defects below 10 % of a tensor are fp32 coverage.
# K: the next power of two at or above twice the worst HIP ratio measured on the MI355X,
# err_hip / max(err_torch, floor) as tensor / row / column / zeros:
#   A fp32   1.29 blocks.11.norm1.bias / 1.70 blocks.9.attn.qkv.weight[q] / 1.98 classifier.3.weight / 0.69
#   B fp32   1.12 blocks.0.attn.qkv.bias[q] / 1.84 gcn.fc2.weight / 1.15 blocks.0.mlp.fc2.weight / 0.56
#   C fp32   1.01 blocks.1.attn.qkv.bias[q] / 1.45 blocks.0.attn.proj.weight / 1.49 blocks.2.attn.proj.weight / 1.05
#   -> worst 1.98, twice is 3.96: K_VIT = 4, below the smallest planted-defect margin of test_grad_checker.py
#      (21, one fc2.weight column x 1.0004, a scale only the column rule rejects; the next is 1062;
#      VIT_DEFECT_CAP = 16 there).
#   A bf16   1.02 blocks.10.norm1.weight / 1.40 blocks.1.attn.proj.weight / 1.32 blocks.9.mlp.fc2.weight / 1.00
#   B bf16   1.13 classifier.3.weight / 1.30 blocks.0.attn.qkv.weight[q] / 1.47 classifier.3.weight / 1.74
#   C bf16   1.91 blocks.2.norm1.bias / 3.03 blocks.1.attn.qkv.weight[q] / 1.80 blocks.1.attn.qkv.weight[k] / 1.97
#   D bf16   1.01 norm.weight / 1.49 blocks.0.attn.qkv.weight[k] / 1.20 classifier.3.weight / 0.77
#   -> worst 3.03, twice is 6.06: K_VIT_BF16 = 8.
VIT_TENSOR_FLOOR = 5e-7
VIT_ROW_FLOOR = 3.8e-6
VIT_COL_FLOOR = 9e-6
VIT_ZERO_FLOOR = 8e-9
VIT16_TENSOR_FLOOR = 1e-2
VIT16_ROW_FLOOR = 1e-1
VIT16_COL_FLOOR = 8e-2
VIT16_ZERO_FLOOR = 5e-5
K_VIT = 4.0
K_VIT_BF16 = 8.0

_RUN = {}


def class_weights(nc):
    """CLASS_W of b0_helpers.py (0.7, 1.3) stretched to nc classes"""
    return torch.linspace(0.7, 1.3, nc)


def adjacency(case):
    """A_norm (B, N, N).  'sym': D^-1/2 (A + I) D^-1/2 of a path graph (symmetric, as the reference builds
    it); 'asym': random positive entries, every row divided by its sum (not symmetric: the head backward's
    transposed mix differs from the plain one)."""
    c = CASES[case]
    b, n = c["B"], c["N"]
    if c["adj"] == "asym":
        g = torch.Generator().manual_seed(SEED + 2)
        a = torch.rand(b, n, n, generator=g) + 0.1
        return a / a.sum(dim=2, keepdim=True)
    a = torch.eye(n)
    for i in range(n - 1):
        a[i, i + 1] = a[i + 1, i] = 1.0
    a[0, 0] = 2.0  # unequal degrees, still symmetric
    d = a.sum(dim=1).rsqrt()
    return (d[:, None] * a * d[None, :]).expand(b, n, n).contiguous()


def inputs(case, layout="contiguous"):
    """(images (B, N, 3, 224, 224), A_norm, labels, class weights); layout 'channels_last': the same values
    with channels-last strides over the last three dims (sw = 3, sc = 1)"""
    c = CASES[case]
    b, n, nc = c["B"], c["N"], c["classes"]
    x = bh.frames(SEED + 1, (b, n, 3, 224, 224))
    if layout == "channels_last":
        x = x.reshape(b * n, 3, 224, 224).contiguous(memory_format=torch.channels_last).view(b, n, 3, 224, 224)
        assert not x.is_contiguous()
    labels = torch.tensor([(i * 7 + 1) % nc for i in range(b)])
    return x, adjacency(case), labels, class_weights(nc)


def _plain_model(case):
    c = CASES[case]
    m = DeepfakeModelCPU(gcn_hid=c["hid"], gcn_out=c["out"], num_classes=c["classes"], depth=c["depth"])
    deterministic_init_(m, seed=SEED)
    m.gcn.dropout.p = 0.0
    m.classifier[2].p = 0.0
    return m.train()


# The classifier's ReLU (classifier.1) sees one pre-activation per clip and unit: 1 - 3 values per unit.  A unit
# whose pre-activation lies within the bf16 step's feature error of zero is alive in one run and dead in the
# other: the gradient is then not a smooth function of the features, the premise of "err <= K x torch's error"
# fails (one flipped unit is 1/B of its bias gradient, and a classifier.0.weight row that is exactly zero in
# fp64 is not), and the outcome says nothing about a kernel.  As the CNN-LSTM cases assert that the max-pool
# argmaxes agree, every case here asserts a margin, from the oracle alone: with z the fp64 classifier.0
# pre-activations and z_ac the same fp64 head applied to the features of torch's bf16 autocast trunk,
#     |z| >= K_VIT_BF16 x max |z_ac - z|     for every clip and unit
# -- no step within K_VIT_BF16 x autocast's feature error can flip a unit.  The plain deterministic_init_ does
# not meet it: on the MI355X case A's smallest |z| was 3.8e-3 where the HIP bf16 features move z by up to 2.3e-2,
# one unit of 128 flipped, and classifier.0.bias came out 0.496 off (autocast: 3.2e-3), a classifier.0.weight
# row that is exactly zero in fp64 non-zero.  So each unit's classifier.0.bias is shifted by the smallest
# multiple of band / 4 that clears the band for all of its clips (``cls_margin``; applied to every run of a
# case, oracle and HIP, fp32 and bf16 alike).  The GCN's two ReLUs see B x N values per unit in tensors of
# 128 - 256 rows whose bf16 anchors are >= 10 %; they are left as they are (measured flips between the fp64 and
# the HIP bf16 features, gcn.fc1 / gcn.fc2: A 3 / 1, B 0 / 0, C 4 / 1, D 42 / 24 of 18,944 / 9,472 values).
# Measured (band, units shifted of 64): A 0.202, 19; B 0.247, 10; C 0.184, 18; D 0.082, 8; with the shift no
# classifier unit differs between the fp64 and the HIP bf16 features in any case.
CONDITION = True


def _cls_preact(m, feats, a):
    b, n = a.shape[:2]
    return m.classifier[0](m.gcn(feats.view(b, n, -1), a).mean(dim=1))


def cls_margin(case, device=None):
    """(per-unit shift of classifier.0.bias, band, smallest |z| after the shift), cached per case"""
    key = (case, "cls_margin")
    if key not in _RUN:
        import copy
        device = device or ("cuda" if torch.cuda.is_available() else "cpu")
        x, a = inputs(case)[:2]
        x = x.reshape(-1, 3, 224, 224).to(device)
        m = _plain_model(case).double().to(device)
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            z = _cls_preact(m, m.vit(x.double()), a.double().to(device))
            m32 = copy.deepcopy(m).float()
            with torch.autocast(torch.device(device).type, dtype=torch.bfloat16):
                f_ac = m32.vit(x)
            z_ac = _cls_preact(m, f_ac.double(), a.double().to(device))
        z, z_ac = z.cpu(), z_ac.cpu()
        band = K_VIT_BF16 * float((z_ac - z).abs().max())
        steps = torch.arange(0, 401, dtype=torch.float64) * (band / 4)
        grid = torch.stack([steps, -steps], dim=1).flatten()  # 0, -0, s, -s, 2s, -2s, ...
        ok = ((z[None] + grid[:, None, None]).abs() >= band).all(dim=1)  # [grid, unit]
        assert bool(ok.any(dim=0).all())
        shift = grid[ok.float().argmax(dim=0)]
        _RUN[key] = (shift, band, float((z + shift).abs().min()))
    return _RUN[key]


def oracle_model(case):
    """the fp32 oracle module of a case with the step's initial weights (classifier.0.bias shifted by
    ``cls_margin``)"""
    m = _plain_model(case)
    if CONDITION:
        with torch.no_grad():
            m.classifier[0].bias += cls_margin(case)[0].float()
    return m


def split(grads):
    """the gradient dict with every attn.qkv.weight / .bias replaced by its q, k, v slices"""
    out = {}
    for n, g in grads.items():
        if ".attn.qkv." in n:
            for i, s in enumerate("qkv"):
                out[f"{n}[{s}]"] = g[i * E:(i + 1) * E]
        else:
            out[n] = g
    return out


def _run(case, mode, device, prepare=None):
    """one oracle step; mode 'fp64' / 'fp32' / 'autocast'.  Everything returned lives on the CPU.
    ``prepare(model)`` may register hooks on the model before the step and returns their handles (the
    planted defects of test_grad_checker.py)."""
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    x, a, labels, cw = inputs(case)
    dt = torch.float64 if mode == "fp64" else torch.float32
    m = oracle_model(case).to(dt).to(device)
    feats = {}
    hooks = [m.vit.register_forward_hook(lambda _m, _i, o: feats.__setitem__("f", o.detach()))]
    if prepare is not None:
        hooks += list(prepare(m))
    x, a, labels, cw = x.to(device, dt), a.to(device, dt), labels.to(device), cw.to(device, dt)
    with torch.backends.cudnn.flags(enabled=False):
        if mode == "autocast":
            with torch.autocast(torch.device(device).type, dtype=torch.bfloat16):
                logits = m(x, a)
            logits = logits.float()
        else:
            logits = m(x, a)
        loss = F.cross_entropy(logits, labels, weight=cw)
        loss.backward()
    for k in hooks:
        k.remove()
    return dict(logits=logits.detach().cpu(), loss=float(loss.detach()), feats=feats["f"].float().cpu() if
                mode == "autocast" else feats["f"].cpu(),
                grads={n: p.grad.detach().cpu() for n, p in m.named_parameters()})


def oracle(case, mode="fp32", device="cpu"):
    key = (case, mode)
    if key not in _RUN:
        _RUN[key] = _run(case, mode, device)
    return _RUN[key]


def anchor(case, mode="fp32", device="cpu"):
    """grad_errors (tensor, row, column) of torch's own fp32 / autocast step against the fp64 one"""
    key = (case, mode, "anchor")
    if key not in _RUN:
        _RUN[key] = bh.grad_errors(split(oracle(case, mode, device)["grads"]),
                                   split(oracle(case, "fp64", device)["grads"]), columns=True)
    return _RUN[key]


def floors(dtype):
    """(K, tensor, row, column, zero floor) of the fp32 / bf16 rule"""
    if dtype == "fp32":
        return K_VIT, VIT_TENSOR_FLOOR, VIT_ROW_FLOOR, VIT_COL_FLOOR, VIT_ZERO_FLOOR
    return K_VIT_BF16, VIT16_TENSOR_FLOOR, VIT16_ROW_FLOOR, VIT16_COL_FLOOR, VIT16_ZERO_FLOOR


def grad_violations(got, case, dtype="fp32", device="cpu", k=None, tag="", columns=True):
    """``got`` ({name: gradient}, unsplit) by the anchored rule; the named structural zeros are bounded by
    ||g|| <= K x max(||g_torch||, zero floor x scale), scale = the largest fp64 gradient norm.
    Returns (violations, worst tensor, row, column and structural-zero ratio).  ``columns=False`` leaves
    the column rule out (what the B0 / CNN-LSTM checker would see)."""
    mode = "fp32" if dtype == "fp32" else "autocast"
    kk, tf, rf, cf, zf = floors(dtype)
    k = kk if k is None else k
    g64 = split(oracle(case, "fp64", device)["grads"])
    gt = split(oracle(case, mode, device)["grads"])
    got = split(got)
    zs = zeros(case)
    assert sorted(got) == sorted(g64) and zs <= set(g64)
    res = bh.grad_bound_violations(got, g64, anchor(case, mode, device), k=k, tag=f"vit {case}/{dtype}{tag}",
                                   tensor_floor=tf, channel_floor=rf, skip=zs, column_floor=cf if columns else None)
    bad, wt, wr = res[:3]
    wc = res[3] if columns else 0.0
    scale = max(float(r.norm()) for r in g64.values())
    wz = 0.0
    for n in sorted(zs):
        a = max(float(gt[n].double().norm()), zf * scale)
        z = float(got[n].double().norm())
        wz = max(wz, z / a)
        if not z <= k * a:
            bad.append((n, "zero", z / scale, float(gt[n].double().norm()) / scale))
    print(f"vit {case}/{dtype}{tag} structural zeros: worst ||g|| / max(||g_torch||, floor) = {wz:.3f}")
    return bad, wt, wr, wc, wz


def feature_violations(feats, case, dtype="fp32", device="cpu", tag=""):
    """the (images, 768) CLS features by the same anchored rule (tensor, image row, feature column)"""
    mode = "fp32" if dtype == "fp32" else "autocast"
    k, tf, rf, cf, _ = floors(dtype)
    f64 = {"features": oracle(case, "fp64", device)["feats"]}
    an = bh.grad_errors({"features": oracle(case, mode, device)["feats"]}, f64, columns=True)
    bad, wt, wr, wc = bh.grad_bound_violations({"features": feats}, f64, an, k=k, tag=f"vit {case}/{dtype}{tag}",
                                               tensor_floor=tf, channel_floor=rf, skip=frozenset(), column_floor=cf)
    return bad, max(wt, wr, wc)


def hip_step(case, dtype, cuda, layout="contiguous"):
    """the same step on the HIP model: (logits, loss, {gradients}) on the CPU"""
    from deepfake_amd.vit_gcn import DeepfakeModel
    c = CASES[case]
    x, a, labels, cw = inputs(case, layout)
    m = DeepfakeModel(gcn_hid=c["hid"], gcn_out=c["out"], num_classes=c["classes"], compute_dtype=dtype,
                      depth=c["depth"])
    m.load_state_dict(oracle_model(case).state_dict())
    m.gcn.dropout.p = 0.0
    m.classifier[2].p = 0.0
    m = m.to(cuda).train()
    logits = m(x.to(cuda), a.to(cuda))
    loss = F.cross_entropy(logits, labels.to(cuda), weight=cw.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters()}
    return logits.detach().cpu(), float(loss.detach()), grads


def hip_features(case, dtype, cuda):
    """ViTFeatureExtractor with the case's ViT weights on the case's images: (images, 768) on the CPU"""
    from deepfake_amd.vit_gcn import ViTFeatureExtractor
    c = CASES[case]
    x = inputs(case)[0]
    fx = ViTFeatureExtractor(compute_dtype=dtype, depth=c["depth"])
    fx.load_state_dict(oracle_model(case).vit.state_dict())
    fx = fx.to(cuda)
    with torch.no_grad():
        f = fx(x.reshape(-1, 3, 224, 224).to(cuda))
    torch.cuda.synchronize()
    return f.float().cpu()
