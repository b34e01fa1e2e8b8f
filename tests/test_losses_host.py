"""FocalLoss / SmoothedCrossEntropyLoss / ImprovedTrainStep without a GPU.

* ``loss_helpers.focal_loss`` / ``smoothed_ce`` (the oracle of ``test_losses_gpu.py``) against
  ``tests/golden/improved_losses.npz``: the reference's ``FocalLoss`` and torch's ``nn.CrossEntropyLoss`` in fp32
  over the whole grid of ``loss_helpers.py``.  The restatement sums in another order (closed form on the label's
  entry, ``logsumexp`` instead of ``log_softmax``), so it differs by a few ulp.  Measured over every loss (per
  row, mean, sum) and every ``dlogits`` of the grid, the fp32 restatement against the reference's fp32 output:
  worst |a - b| = 3.05e-5 (two fp32 ulp of a `sum` loss of 206.9), worst max|a - b| / max|b| per tensor =
  6.53e-7.  The bounds are 4 x those: ``ABS_BOUND`` = 1.3e-4 and ``REL_BOUND`` = 2.7e-6, each for every tensor.
* constructor contracts (the reference's: list / tuple weights, the ``weight`` buffer), bad reductions,
  fake-tensor shapes of the two operators, the C ABI's refusal of C outside [1, 1024], CPU refusal.
"""
import ctypes

import pytest
import torch

import loss_helpers as lh
from deepfake_amd import _lib, ops
from deepfake_amd.losses import FocalLoss, SmoothedCrossEntropyLoss

ABS_BOUND = 1.3e-4
REL_BOUND = 2.7e-6


def test_restatement_matches_reference_golden():
    G = lh.load_golden()
    worst = [0.0, 0.0]

    def hold(got, key):
        ref = G[key].double()
        assert torch.isfinite(ref).all(), key
        d = float((got.double() - ref).abs().max())
        r = d / float(ref.abs().max()) if float(ref.abs().max()) > 0 else 0.0
        worst[0], worst[1] = max(worst[0], d), max(worst[1], r)
        assert d <= ABS_BOUND and r <= REL_BOUND, (key, d, r)

    def case(key, fn, z, *args):
        for red in lh.REDUCTIONS:
            loss, dz = lh.with_grad(fn, z, *args, red)
            hold(loss, f"{key}/{'rows' if red == 'none' else red}")
            if red == "mean":
                hold(dz, f"{key}/dmean")

    n = 0
    for B, C, gamma, eps, wk in lh.focal_cases():
        z, t = G[f"in/{B}x{C}/logits"], G[f"in/{B}x{C}/targets"]
        case(lh.focal_key(B, C, gamma, eps, wk), lh.focal_loss, z, t, gamma, lh.class_weight(wk, t, C), eps)
        n += 1
    for B, C, eps, wk, tk in lh.ce_cases():
        z, t = G[f"in/{B}x{C}/logits"], G[f"in/{B}x{C}/targets"]
        case(lh.ce_key(B, C, eps, wk, tk), lh.smoothed_ce, z, lh.ce_targets(tk, t), lh.class_weight(wk, t, C), eps,
             lh.IGNORE)
        n += 1
    for gamma in (0.0, 2.0):
        case(f"focal/sat/g{gamma}", lh.focal_loss, G["in/sat/logits"], G["in/sat/targets"], gamma, None, 0.0)
    print(f"{n} cases: worst |a - b| {worst[0]:.3e} (bound {ABS_BOUND}), worst relative {worst[1]:.3e} "
          f"(bound {REL_BOUND})")
    assert n == 141 + 78


def test_golden_inputs_are_the_grid():
    G = lh.load_golden()
    for B, C in lh.SHAPES:
        z, t = lh.shape_inputs(B, C)
        assert torch.equal(G[f"in/{B}x{C}/logits"], z) and torch.equal(G[f"in/{B}x{C}/targets"], t)


def test_gamma_half_cases_are_away_from_pt_one():
    """the reference itself is finite on the gamma = 0.5 cases: 1 - pt > 1e-4 on every row"""
    for B, C, gamma, eps, _ in lh.focal_cases():
        if gamma == 0.5:
            z, t = lh.shape_inputs(B, C)
            assert float((1.0 - lh.focal_pt(z.double(), t, eps)).min()) > 1e-4, (B, C, eps)


def test_constructor_contracts():
    f = FocalLoss()
    assert (f.gamma, f.weight, f.label_smoothing, f.reduction) == (2.0, None, 0.0, "mean")
    assert "weight" in f._buffers  # registered even when None, as in the reference
    f = FocalLoss(gamma=1.5, weight=[0.25, 0.75], label_smoothing=0.1, reduction="sum")
    assert f.weight.dtype == torch.float32 and f.weight.tolist() == [0.25, 0.75]
    assert "weight" in f.state_dict() and dict(f.named_buffers())["weight"] is f.weight
    assert FocalLoss(weight=(1, 2)).weight.tolist() == [1.0, 2.0]
    w64 = torch.tensor([1.0, 3.0], dtype=torch.float64)
    c = SmoothedCrossEntropyLoss(weight=w64, label_smoothing=0.2, ignore_index=7, reduction="none")
    assert c.weight.dtype == torch.float32 and c.weight.data_ptr() != w64.data_ptr()
    assert (c.label_smoothing, c.ignore_index, c.reduction) == (0.2, 7, "none")
    assert SmoothedCrossEntropyLoss().ignore_index == -100
    for cls in (FocalLoss, SmoothedCrossEntropyLoss):
        with pytest.raises(ValueError):
            cls(reduction="batchmean")
        with pytest.raises(ValueError):
            cls(label_smoothing=1.0)


def test_ops_registered_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert not set(ops.LOSS_OPS) & set(ops.OPS)
    for name in ops.LOSS_OPS:
        assert getattr(torch.ops.dfd, name).default._schema.name == f"dfd::{name}"
    assert "Tensor? weight" in str(torch.ops.dfd.classification_loss.default._schema)
    with FakeTensorMode():
        z, t = torch.empty(7, 5), torch.empty(7, dtype=torch.long)
        for red, shape in (("mean", ()), ("sum", ()), ("none", (7,))):
            loss, work = torch.ops.dfd.classification_loss(z, t, None, "focal", red, 2.0, 0.1, -100)
            assert loss.shape == shape and loss.dtype == torch.float32
            assert work.shape == (7 * 5 + 4 * 7 + 1,)
            d = torch.ops.dfd.classification_loss_backward(torch.empty(shape), t, torch.empty(5), work, 5, "ce", red,
                                                           0.0, 0.1, -100)
            assert d.shape == (7, 5) and d.dtype == torch.float32


def test_launcher_refuses_class_counts_outside_1_to_1024():
    lib = _lib.load()
    assert lib.dfd_loss_work_floats(3, 1024) == 3 * 1024 + 13
    assert lib.dfd_loss_work_floats(3, 1025) == -1 and lib.dfd_loss_work_floats(3, 0) == -1
    buf = ctypes.create_string_buffer(64)  # never dereferenced: the launcher refuses before any launch
    p = ctypes.addressof(buf)
    for C in (0, 1025):
        assert lib.dfd_loss_forward(None, 0, 1, p, p, None, 2, C, 2.0, 0.0, -100, p, p) == -1
        assert b"1 <= C <= 1024" in lib.dfd_last_error()
        assert lib.dfd_loss_backward(None, 1, 1, p, None, 2, C, 2.0, 0.0, -100, p, p, p) == -1
    assert lib.dfd_loss_forward(None, 2, 1, p, p, None, 2, 2, 2.0, 0.0, -100, p, p) == -1  # unknown mode
    assert lib.dfd_loss_forward(None, 0, 1, p, p, None, 2, 2, 2.0, 1.0, -100, p, p) == -1  # smoothing of 1


def test_cpu_tensors_refused():
    z, t = torch.zeros(2, 2), torch.zeros(2, dtype=torch.long)
    for crit in (FocalLoss(), SmoothedCrossEntropyLoss(label_smoothing=0.1)):
        with pytest.raises(RuntimeError):
            crit(z, t)
    with pytest.raises(NotImplementedError):
        torch.ops.dfd.classification_loss(z, t, None, "focal", "mean", 2.0, 0.0, -100)


def test_improved_train_step_rejects_unknown_loss():
    from deepfake_amd.trainer import ImprovedTrainStep

    cfg = dict(learning_rate=1e-3, weight_decay=1e-2, max_epochs=5, class_weights=[1.0, 1.0], loss="hinge")
    with pytest.raises(ValueError):
        ImprovedTrainStep(torch.nn.Linear(2, 2), cfg)
