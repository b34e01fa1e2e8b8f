"""Every element of every LogicRNNLSTM gradient, with dropout on, at the shapes the model had never run at.

One training step (``rnn_helpers.hip_step``: ``deterministic_init_`` with the attention rescale, BCE against
targets in sorted row order, backward) against the restated ``LogicRNNLSTMCPU`` of ``rnn_helpers.py`` on the
CPU.  The oracle gets the sort permutation the device itself takes (``lengths.to(cuda).sort``; tie order is
the device's) and the dropout keep-scales of the library's counter hash restated in NumPy, so with p > 0
``y`` and the loss at rtol 1e-4 / atol 1e-6 against the fp32 oracle pin the hash, the stream ids and the
element indices, and every gradient element is judged by the whole-tensor checker
(``rnn_helpers.grad_violations``: per tensor and per dim-0 row, u-gate weights as x- and h-column blocks,
err <= K_RNN x max(torch-fp32's own error, floor), both against the fp64 oracle; named structural zeros bounded
in norm).  Each case runs with the per-cell launches (``rnn_step``, k_rnn_step.hip) on and -- where the hidden
size is step-supported -- off (the K-sliced products + cell kernels of k_rnn.hip).

Cases (B x T x IN, hidden H, L layers, lengths, p) and what the launch arithmetic gives.  Step path: forward
grid H/2 workgroups, rows in chunks of 64 (4 waves x 16 MFMA rows), NS = H/16 A-operand float4 per lane,
WV = H/64 weight float4 per thread; backward product rnn_dh_kernel (H/16) x 8 workgroups, kc = 7H/8 k per
slice, PV = ceil(kc*4 / 256) float4 per thread.  Sliced path: sgemm_splits(M, N, K) = min(256 / tiles, K/64,
64) slices of 64 x 64 tiles, forward h.P^T (M = B, N = 7H, K = H), backward dz.P (M = B, N = H, K = 7H).
Both: x projection M = B*T, N = 6H, K = IN and weight gradients dP (M = 7H, N = H, K = B*T), dWX0 (M = 6H,
N = IN, K = B*T) -- no case here meets the 128 x 64 big-tile conditions (B*T % 32 != 0 or % 128 != 0), so
all run sgemm_kernel's ragged 64 x 64 tiles, sgemm_wsplits = 1 slice (B*T < 512).

``h128b5``  5x3x40, 128, 2, lengths 3 1 2 5 4 (distinct; 4 and 5 > T count as full), p 0: one partial MFMA row
  block (rows 5 .. 15 zero A operands, waves 1 - 3 all zero); IN = 40: x projection K = 40 (2.5 k-steps of
  16), dWX0 N = 40 (one ragged column tile); kc = 112, PV = 2 (448 of 512 float4 slots).  Sliced: forward 14
  column tiles x 2 slices of 64; backward 2 tiles x 14 slices of 64.
``h256b70`` 70x2x64, 256, 3, lengths 1 / 2 tied 35 : 35, p 0.3: second 64-row chunk of 6 rows in both step
  kernels; a middle layer (dcl read and written in place, dropout streams 0 and 1); classifier dropout
  (stream 9).  kc = 224, PV = 4 (896 of 1024).  Sliced: M = 70 is 2 row tiles (the second 6 rows): forward
  28 x 2 tiles, 4 slices of 64; backward 4 x 2 tiles, 28 slices of 64.
``h384``    17x4x96, 384, 1, lengths 1 .. 4, p 0: L = 1 (the last layer is layer 0: dc in place, no inter-layer
  dropout); two MFMA row blocks, the second with one row; WV = 6; kc = 336, kc*4 = 1344 = 5.25 x 256: PV = 6
  with the last pass ragged (the only such size).  Sliced: forward 42 tiles x 6 slices of 64; backward 6
  tiles x 42 slices of 64.
``h512``    33x2x128, 512, 2, no lengths, p 0.5: the bench hidden size; order == nullptr with dropout on
  (mask index row = b*T + t in clip order); three MFMA row blocks (the third one row).  Sliced: forward 56
  tiles x 4 slices of 128; backward 8 tiles x 32 slices of 112.
``h72``     3x5x48, 72, 2, lengths 7 2 4 (7 > T, as detector.py passes them un-clamped), p 0.3: not
  step-supported (one knob setting).  N = 504 forward: 8 column tiles, the last 56 wide, K = 72 in 1 slice of
  80 (4.5 k-steps); backward N = 72: 2 column tiles (the last 8 wide), K = 504 in 7 slices of 80 (the last
  24); attention / classifier GEMMs N = 72.
``t1``      4x1x32, 128, 2, lengths 1 3 1 2, p 0: no recurrent flow (the last layer's dh_b == nullptr, no
  product into step 0's h = 0), softmax over one element.  Structural zeros, 13 of 48 judged tensors (27 %;
  every other case 1 of 28 .. 68): attention.{0,2}.{weight,bias}, logic_cells.0.not_gate.weight, the h-column
  block of layer 0's six u-gates, and -- c = 0 enters layer 0 -- logic_cells.0.forget_gate.bias and
  forget_gate.weight[x].  All are bounded in norm.
``nolen``   6x3x32, 128, 2, lengths None, p 0: order == nullptr (dWX0 reads x itself, no gather), mask off.
``test_eval_forward_is_train_forward_without_dropout``: h256b70 in ``eval()`` at p = 0.3 equals the train-mode
  forward of a p = 0 model bit for bit.

Measured on the MI355X, err_hip / max(err_torch_fp32, floor) as (worst tensor, worst dim-0 row, worst column
block, structural zeros), rnn_step on / off:
  case      rnn_step on                    rnn_step off (K-sliced)
  h128b5    0.25 / 0.10 / 0.17 / 0.060     0.15 / 0.08 / 0.27 / 0.024
  h256b70   0.20 / 0.07 / 0.18 / 0.005     0.20 / 0.07 / 0.20 / 0.001
  h384      0.75 / 0.19 / 0.67 / 0.018     1.18 / 0.27 / 1.06 / 0.016
  h512      0.35 / 0.10 / 0.27 / 0.032     0.30 / 0.08 / 0.23 / 0.016
  h72       --                             0.19 / 0.09 / 0.20 / 0.186
  t1        0.09 / 0.04 / 0.48 / 0.000     0.10 / 0.04 / 0.31 / 0.000
  nolen     0.39 / 0.11 / 0.24 / 0.050     0.42 / 0.09 / 0.25 / 0.088
The worst, 1.18, is attention.0.weight at h384 off (3.5e-6 against torch's 1.1e-6, under the 3e-6 floor;
attention.2.weight 3.4e-6, logic_cells.0.not_gate.weight 3.2e-6, the six layer-0 h-column blocks 3.0e-6 ..
3.2e-6): T = 4 is the longest recurrence here and H = 384 the 42-slice backward product.  Twice 1.18 is 2.4:
K_RNN = 4 (``rnn_helpers.py``).  (With the floors at half their value, before they were doubled for machines
with another CPU thread count, the same run gave 2.35.)  y differs from the fp32 oracle by at most one ulp
(6e-8) and the loss by 2e-7 relative in every run, dropout cases included.  Each run takes 0.05 - 0.5 s.
"""
import pytest
import torch

import rnn_helpers as rh

pytestmark = pytest.mark.gpu

RUNS = [(c, s) for c in rh.CASES for s in ((True, False) if rh.dims(c)[3] in rh.STEP_H else (False,))]


def _cpu_condition(case):
    p = rh.dims(case)[5]
    if p > 0:
        for m in (lambda i, c: i + [c])(*rh.masks(case)):
            share, ok = rh.keep_share_ok(m, p)
            assert ok, (case, share)
    assert case == "t1" or rh.skipped_share(case) < rh.bh.MAX_SKIPPED


@pytest.mark.parametrize("case,step", RUNS, ids=[f"{c}-{'step' if s else 'sliced'}" for c, s in RUNS])
def test_train_step_every_gradient_element(cuda, case, step):
    _cpu_condition(case)
    prev = rh.set_step_knob(step)
    try:
        y, loss, grads = rh.hip_step(case, cuda)
    finally:
        rh.set_step_knob(prev)
    perm = rh.device_perm(case, cuda)
    ref = rh.oracle(case, perm)
    print(f"{case} step={step}: loss {loss:.7f} oracle {ref['loss']:.7f}; max |y - y_ref| "
          f"{float((y - ref['y']).abs().max()):.2e}")
    torch.testing.assert_close(y, ref["y"], rtol=1e-4, atol=1e-6)
    assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"]) + 1e-6
    bad, wt, wr, wb, wz = rh.grad_violations(grads, case, perm, tag=f" step={int(step)}")
    print(f"{case} step={step}: worst tensor {wt:.2f}, row {wr:.2f}, column block {wb:.2f}, zeros {wz:.3f}")
    assert not bad, bad[:12]


def test_eval_forward_is_train_forward_without_dropout(cuda):
    case = "h256b70"
    x, lengths, _ = rh.inputs(case)
    x, lengths = x.to(cuda), lengths.to(cuda)
    for step in (True, False):
        prev = rh.set_step_knob(step)
        try:
            with torch.no_grad():
                y_eval = rh.hip_model(case, cuda, p=0.3).eval()(x, lengths)
            y_train = rh.hip_model(case, cuda, p=0.0).train()(x, lengths)
        finally:
            rh.set_step_knob(prev)
        assert torch.equal(y_eval.cpu(), y_train.detach().cpu()), step
