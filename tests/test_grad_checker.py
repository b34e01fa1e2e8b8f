"""Self-test of the whole-tensor fp32 gradient checker (``b0_helpers.grad_errors`` /
``grad_bound_violations``) on the CPU: torch's own fp32 gradients of the oracle step stand in for the HIP
ones, at the smallest shape of ``test_b0_grad_full_gpu.py`` (1 clip x 3 frames x 100x84).

* the unmodified fp32 gradients pass;
* every planted defect -- each of a size a kernel that is wrong in one channel tile, one tail tile or one
  tap would produce, and each invisible to "norm within 1e-3 + 64 leading elements" -- is rejected, on a
  1x1 weight (the first expansion, 96x16, and conv_head, 1280x320), a k3 and a k5 depthwise weight and a
  BN weight.

This caps ``K32`` and the floors: a defect is rejected only while its error exceeds
K32 x max(torch-fp32 error, floor), so every defect's margin (error / that anchor, printed) must stay
above K32.  Measured margins (seed 21): the smallest is 59 (the BN weight's last element x 1.02, a
5.9e-4 change of the tensor), every weight-row defect is above 200: K32 may not exceed 32.
"""
import pytest
import torch

import b0_helpers as bh

SHAPE = (1, 3, 100, 84)
PW = ["backbone.2.1.0.conv_pw.weight", "backbone.3.weight"]
DW = ["backbone.2.1.1.conv_dw.weight", "backbone.2.2.0.conv_dw.weight"]  # k3, k5 (144 channels each)
BN = ["backbone.2.1.0.bn1.weight"]


def scale_last(g):
    g[-1] *= 1.02


def swap_channels(g):
    a, b = 1, g.shape[0] // 2
    g[[a, b]] = g[[b, a]]


def zero_tap(g):
    g[g.shape[0] // 3, 0, 0, -1] = 0.0


def transpose_taps(g):
    c = 2 * g.shape[0] // 3
    g[c, 0] = g[c, 0].t().clone()


def zero_late_element(g):
    f = g.view(-1)
    f[f.numel() - 1 - f.numel() // 16] = 0.0  # the middle of the last eighth


DEFECTS = ([(n, d) for n in PW + DW + BN for d in (scale_last, swap_channels, zero_late_element)]
           + [(n, d) for n in DW for d in (zero_tap, transpose_taps)])


@pytest.fixture(scope="module")
def step():
    return bh.oracle_step(SHAPE)["grads"], bh.oracle64_step(SHAPE), bh.fp32_anchor(SHAPE)


def test_shapes_of_the_planted_tensors(step):
    g32, _, _ = step
    assert [tuple(g32[n].shape) for n in PW] == [(96, 16, 1, 1), (1280, 320, 1, 1)]
    assert [tuple(g32[n].shape) for n in DW] == [(144, 1, 3, 3), (144, 1, 5, 5)]
    assert tuple(g32[BN[0]].shape) == (96,)


def test_unmodified_fp32_gradients_pass(step):
    g32, g64, anchor = step
    bad, wt, wc = bh.grad_bound_violations(g32, g64, anchor, tag="torch fp32")
    assert not bad, bad
    assert wt <= 1.0 and wc <= 1.0  # its own anchor
    # and the same through the entry point the GPU tests use
    bh.check_grads_full(g32, SHAPE, " torch fp32")


def test_old_check_misses_a_late_channel(step):
    """what the checker is for: the last output channel of conv_head off by 2 % passes the norm (1e-3)
    and leading-64 checks of the earlier fp32 tests"""
    g32, _, _ = step
    n = "backbone.3.weight"
    g = g32[n].clone()
    scale_last(g)
    assert abs(float(g.norm()) - float(g32[n].norm())) <= 1e-3 * float(g32[n].norm())
    assert torch.equal(g.flatten()[:64], g32[n].flatten()[:64])


@pytest.mark.parametrize("name,defect", DEFECTS, ids=[f"{n}-{d.__name__}" for n, d in DEFECTS])
def test_planted_defect_is_rejected(step, name, defect, capsys):
    g32, g64, anchor = step
    got = dict(g32)
    got[name] = g32[name].clone()
    defect(got[name])
    assert not torch.equal(got[name], g32[name])
    bad, wt, wc = bh.grad_bound_violations(got, g64, anchor, tag=f"{name} {defect.__name__}")
    capsys.readouterr()  # the worst-six report is not of interest here
    print(f"{name} {defect.__name__}: margin {max(wt, wc):.1f} (K32 = {bh.K32})")
    assert bad and all(b[0] == name for b in bad), bad
