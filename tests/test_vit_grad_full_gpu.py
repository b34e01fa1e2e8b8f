"""Every element of every DeepfakeModel (ViT-B/16 + SimpleGCN) gradient, fp32 and bf16.

One training step per case (``vit_helpers.hip_step``: ``deterministic_init_``, head dropout 0, weighted CE,
backward) against ``oracle.vit_cpu.DeepfakeModelCPU`` run as plain PyTorch on the GPU with MIOpen off, in
fp64 (the reference), fp32 (the fp32 anchor) and under torch's bf16 autocast (the bf16 anchor).  fp32 logits
and loss at rtol 1e-3 against the fp32 oracle; every gradient element by ``vit_helpers.grad_violations``:
per tensor, per dim-0 row and per dim-1 column, err <= K x max(torch's own error, floor), both against fp64;
``attn.qkv`` judged as its q, k and v slices; the key-bias slices (structural zeros) bounded in norm.
``K_VIT`` / ``K_VIT_BF16``, the floors and the measured worst ratios are in ``vit_helpers.py`` and DESIGN.md.
Every tensor is judged in bf16 as well: no share of them may fail.

Cases (clips x nodes, depth; 224 x 224 images, 197 tokens per image, M = 197 x images token rows):

``A`` 2 x 3, depth 12 -- the golden's shape at full depth; M = 1182.
``B`` 1 x 1, depth 1 -- M = 197, below one 256-row GEMM tile; ``tokens_bwd`` runs its tail loop only; the
  LayerNorm backward runs cdiv(197, 16) = 13 workgroups; ``A_norm`` is 1 x 1.
``C`` 3 x 3, depth 3, 3 classes, gcn_hid 200, gcn_out 72 (no multiples of 64; ``launch_sgemm`` takes them) --
  an odd depth (the bf16 backward's parity buffers wrap), 9 = 8 + 1 images in ``tokens_bwd``, and a
  row-normalised ``A_norm`` that is not symmetric, so the head backward's transposed mix matters.  Run twice,
  from a contiguous image tensor and from a channels-last view of the same values: bit-identical.
``D`` 2 x 37, depth 1, bf16 -- 74 images, M = 14578: ``vgemm_nt_bn`` picks the 256-wide tile when
  cdiv(M, 256) x (N / 256) >= 512, i.e. 57 x 9 = 513 for qkv (N = 2304; 73 images is the smallest count that
  gives 57 row tiles) and 57 x 12 for fc1 (N = 3072); the 768-wide products stay on the 128-wide tile.

Before the GPU is judged each test asserts the oracle-side condition of ``vit_helpers.cls_margin``: no
classifier.0 pre-activation lies within K_VIT_BF16 x torch-autocast's perturbation of zero (the classifier ReLU
sees 1 - 3 values per unit; a flipped unit makes the gradient a non-smooth function of the features).

Measured on the MI355X, err_hip / max(err_torch, floor) as tensor / row / column / zeros: A fp32 1.29 / 1.70 /
1.98 / 0.69; B fp32 1.12 / 1.84 / 1.15 / 0.56; C fp32 1.01 / 1.45 / 1.49 / 1.05 (K_VIT = 4); A bf16 1.02 / 1.40 /
1.32 / 1.00; B bf16 1.13 / 1.30 / 1.47 / 1.74; C bf16 1.91 / 3.03 / 1.80 / 1.97; D bf16 1.01 / 1.49 / 1.20 / 0.77
(K_VIT_BF16 = 8).  Case C gives the same bits from both layouts.  Each case runs in 0.3 - 5 s.

``ViTFeatureExtractor`` features of cases B and C are judged element-wise by the same anchored rule.
"""
import pytest
import torch

import vit_helpers as vh

pytestmark = pytest.mark.gpu

RUNS = [(c, d) for c in "ABCD" for d in vh.CASES[c]["dtypes"]]


@pytest.mark.parametrize("case,dtype", RUNS, ids=[f"{c}-{d}" for c, d in RUNS])
def test_train_step_every_gradient_element(cuda, case, dtype):
    _, band, least = vh.cls_margin(case)
    print(f"vit {case}: classifier.0 margin band {band:.3e}, smallest |z| {least:.3e}")
    assert least >= band * (1 - 1e-6)
    ref = vh.oracle(case, "fp32", cuda)
    logits, loss, grads = vh.hip_step(case, dtype, cuda)
    print(f"vit {case}/{dtype}: loss {loss:.6f} (torch fp32 {ref['loss']:.6f}), logits {logits.flatten().tolist()}")
    if dtype == "fp32":
        torch.testing.assert_close(logits, ref["logits"], rtol=1e-3, atol=1e-5)
        assert abs(loss - ref["loss"]) <= 1e-3 * abs(ref["loss"]) + 1e-5
    else:  # the bound of test_vit_gcn_bf16_close
        assert abs(loss - ref["loss"]) <= 3e-2 * abs(ref["loss"])
    bad, wt, wr, wc, wz = vh.grad_violations(grads, case, dtype, cuda)
    print(f"vit {case}/{dtype}: worst ratios tensor {wt:.2f}, row {wr:.2f}, column {wc:.2f}, zeros {wz:.3f}")
    assert not bad, bad[:12]
    if case == "C":
        l2, loss2, g2 = vh.hip_step(case, dtype, cuda, "channels_last")
        assert torch.equal(l2, logits) and loss2 == loss
        assert all(torch.equal(g2[n], grads[n]) for n in grads)


@pytest.mark.parametrize("case,dtype", [(c, d) for c in "BC" for d in ("fp32", "bf16")])
def test_features_every_element(cuda, case, dtype):
    bad, worst = vh.feature_violations(vh.hip_features(case, dtype, cuda), case, dtype, cuda)
    print(f"vit {case}/{dtype} features: worst ratio {worst:.2f}")
    assert not bad, bad
