"""Every element of every CNNLSTMHybrid gradient, at the shapes the step had never run at.

One training step (``cnn_lstm_helpers.hip_step``: dropout 0, ``deterministic_init_`` with the attention
rescale, CE loss, backward) against ``oracle.detector_cpu.CNNLSTMHybridCPU`` on the CPU: logits and loss at
rtol 1e-3 / atol 1e-5 against the fp32 oracle; every gradient element by the whole-tensor checker
(``cnn_lstm_helpers.grad_violations``: per tensor and per dim-0 row, err <= K_CL x max(torch-fp32's own
error, floor), both against the fp64 oracle; the named structural zeros bounded in norm); the BN running
statistics after the step by the same anchored rule (``buf_violations``).  Before the GPU is judged each
test asserts the CPU-side condition that the fp32 and the fp64 oracle agree on every max-pool argmax with a
positive window maximum (ReLU and max-pool are not smooth; gaps recorded in ``cnn_lstm_helpers.py``).

Cases (clips x frames x H x W; hidden, LSTM layers, classes; input layout) and what the launch arithmetic
gives.  Conv rows M = frames x Ho x Wo; conv 1 (3->64 7x7/2) runs conv_gemm 64 x 64 tiles and
conv_wgrad_splits = min(cdiv(M, 256), 682) pixel splits; conv 2..4 run the cg32 loops: forward / dgrad
tiles of 128 rows (256 for the 64-wide data gradient of conv 2), wgrad (tiles, sp, mps) from
cg32_wgrad_split with the 4 Mi-float slab.  LSTM / attention / classifier GEMMs are launch_sgemm at
M = clips x frames (input projections) and M = clips (recurrent steps, classifier).  The recurrent
products are K-sliced by sgemm_splits(M, N, K) = min(256 / tiles, K / 64, 64) slices over 64 x 64 tiles:
hidden 64: forward h.W_hh^T (N = 256, K = 64) 4 column tiles, 1 slice; backward dz.W_hh (N = 64, K = 256)
1 tile, 4 slices of 64.  hidden 72: forward N = 288: 5 column tiles (the last 32 wide), 1 slice; backward
N = 72: 2 column tiles (the last 8 wide), K = 288 in 4 slices.

``cl56`` 2x3x40x56; 64, 2, 2; channels-last -- maps 20x28 -> 10x14 -> 5x7 -> 3x4:
  M = 3360 / 840 / 210 / 72.  conv 1: 53 row tiles (last 32 rows), 14 wgrad splits.  conv 2: 7 forward tiles
  (last 72), dgrad<256,64> on its 840 input rows: 4 tiles (last 72), wgrad 50 tiles x 7 splits of 128 (last 72).
  conv 3: 2 x 2 forward tiles (last 82), dgrad<128,128> 210 rows: 2 tiles, wgrad 72 tiles x 2 (128 + 82).
  conv 4: one partial tile of 72 rows x 4 column tiles, dgrad 72 rows: 1 x 2 tiles, wgrad 288 tiles x 1.
``w100`` 1x5x36x100; 72, 3, 2; channels-last -- maps 18x50 -> 9x25 -> 5x13 -> 3x7: M = 4500 / 1125 / 325 /
  105: 71 conv-1 tiles (last 20 rows), 9 / 3 / 1 forward tiles (last 101 / 69 / 105), wgrad splits 18 / 9 /
  3 / 1.  hidden 72 is no multiple of 64 (4 x 72 = 288 gate columns: a ragged last GEMM column tile), three
  LSTM layers (the dX buffers alternate twice), one clip (recurrent GEMMs of a single row).
``nchw`` 3x2x50x34; 64, 1, 3; plain contiguous NCHW -- maps 25x17 -> 13x9 -> 7x5 -> 4x3: M = 2550 / 702 /
  210 / 72; conv 1 gathers through NCHW strides (OpConvA / OpConvBT with a channel stride of H x W); a
  single LSTM layer (no inter-layer path), three classes (the classifier's N = 3 GEMM and colsum).
``t1`` 2x1x40x56; 72, 2, 2; channels-last -- one frame per clip: no recurrent product, dh == nullptr in every
  LSTM step, softmax over one element; attention.* and lstm.weight_hh_l* are structurally zero there and
  are bounded in norm with the other named zeros (``cnn_lstm_helpers.zeros``).
``min`` 2x2x16x24; 64, 2, 2; channels-last -- the smallest accepted frame: maps 8x12 -> 4x6 -> 2x3 -> 1x2,
  M = 384 / 96 / 24 / 8: every cg32 layer is one partial tile and conv 4's BN normalises over 8 values.  No
  CPU anchor at this size exceeds 1e-3 (worst 6.3e-4, an lstm.weight_hh_l1 row), so the case is not enlarged.
``test_eval_mode_gradients`` -- cl56 in ``eval()`` with gradients enabled (frozen-BN fine-tuning):
  ``launch_bn_bwd_finalize(training = false)``, the conv biases are real gradients through
  ``cl_bias_grad_kernel``; the running statistics (``deterministic_init_``'s hash values: mean 0.1 U,
  var 1 + 0.25 |U|) must not change by a bit.

Measured on the MI355X, err_hip / max(err_torch_fp32, floor) as (worst tensor, worst dim-0 row, structural
zeros, running statistics): cl56 1.08 / 1.03 / 0.12 / 1.01; w100 6.16 (attention.0.weight) / 4.17 / 0.11 /
1.01; nchw 8.09 (lstm.weight_hh_l0) / 5.78 / 0.12 / 1.88; t1 1.29 / 1.31 / 0.06 / 1.05; min 1.26 / 1.16 /
0.15 / 1.01; eval 1.64 / 1.99 / 0.005.  K_CL = 32 (``cnn_lstm_helpers.py``).  Each case runs in 0.1 - 0.6 s.
"""
import pytest
import torch

import cnn_lstm_helpers as ch

pytestmark = pytest.mark.gpu


def _cpu_condition(case, mode):
    same, gap = ch.pool_agreement(case, mode)
    print(f"{case}/{mode}: pool argmaxes agree: {same}; smallest relative top-2 gap {gap:.2e}")
    assert same, "the fp32 and fp64 oracle pick different max-pool argmaxes: choose another seed"


@pytest.mark.parametrize("case", list(ch.CASES))
def test_train_step_every_gradient_element(cuda, case):
    _cpu_condition(case, "train")
    ref = ch.oracle(case)
    logits, loss, grads, bufs = ch.hip_step(case, cuda)
    torch.testing.assert_close(logits, ref["logits"], rtol=1e-3, atol=1e-5)
    assert abs(loss - ref["loss"]) <= 1e-3 * abs(ref["loss"]) + 1e-5
    bad_b, _ = ch.buf_violations(bufs, case)
    bad, _, _, _ = ch.grad_violations(grads, case)
    assert not bad_b, bad_b
    assert not bad, bad[:12]


def test_eval_mode_gradients(cuda):
    case = "cl56"
    _cpu_condition(case, "eval")
    ref = ch.oracle(case, "eval")
    logits, loss, grads, bufs = ch.hip_step(case, cuda, "eval")
    torch.testing.assert_close(logits, ref["logits"], rtol=1e-3, atol=1e-5)
    assert abs(loss - ref["loss"]) <= 1e-3 * abs(ref["loss"]) + 1e-5
    for n, b in ref["bufs_before"].items():  # frozen statistics: bit for bit
        assert torch.equal(bufs[n], b), n
        assert torch.equal(ref["bufs"][n], b), n
    bad, _, _, _ = ch.grad_violations(grads, case, "eval")
    assert not bad, bad[:12]
