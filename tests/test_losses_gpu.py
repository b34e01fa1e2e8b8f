"""FocalLoss / SmoothedCrossEntropyLoss (``csrc/k_loss.hip``) and one ``ImprovedTrainStep`` step on the MI355X.

Loss and ``dlogits`` against ``loss_helpers.focal_loss`` / ``smoothed_ce`` run in fp64 on the CPU and against the
reference's own fp32 output (``tests/golden/improved_losses.npz``), both at the project's rtol 1e-3 / atol 1e-5,
over the whole grid of ``loss_helpers.py`` (shapes, gamma, label smoothing, weights, reductions, ignored rows),
plus C = 1024 (the launcher's limit: 16 logits per lane) and a saturated batch.  Further: a device-scalar and
a per-row upstream gradient, bit-reproducibility, ``torch.library.opcheck``, the label guard, and one
``ImprovedTrainStep`` step of ``vit_helpers`` case C against ``oracle_model`` on the CPU.
"""
import pytest
import torch

import loss_helpers as lh
import vit_helpers as vh
from deepfake_amd.losses import FocalLoss, SmoothedCrossEntropyLoss

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-5
_G = {}


def golden():
    if not _G:
        _G.update(lh.load_golden())
    return _G


def close(got, ref, what):
    torch.testing.assert_close(got.detach().cpu().double(), ref.double(), rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def hip(crit, z, t, cuda, upstream=None):
    """(loss, dlogits) of a HIP criterion, on the CPU"""
    zc = z.to(cuda).requires_grad_(True)
    loss = crit.to(cuda)(zc, t.to(cuda))
    loss.backward(torch.ones_like(loss) if upstream is None else upstream.to(cuda))
    return loss.detach().cpu(), zc.grad.cpu()


def check_case(key, crit_of, oracle, z, t, cuda):
    """every reduction of one case against the fp64 restatement and the golden"""
    G = golden()
    for red in lh.REDUCTIONS:
        loss, dz = hip(crit_of(red), z, t, cuda)
        ref_loss, ref_dz = lh.with_grad(oracle, z.double(), red)
        assert loss.shape == ref_loss.shape and dz.shape == z.shape
        close(loss, ref_loss, f"{key} {red} loss vs fp64")
        close(dz, ref_dz, f"{key} {red} dlogits vs fp64")
        if f"{key}/mean" in G:
            close(loss, G[f"{key}/{'rows' if red == 'none' else red}"], f"{key} {red} loss vs golden")
            if red == "mean":
                close(dz, G[f"{key}/dmean"], f"{key} dlogits vs golden")


@pytest.mark.parametrize("B,C", lh.SHAPES + [(3, 1024)], ids=lambda v: str(v))
def test_focal_grid(cuda, B, C):
    z, t = lh.shape_inputs(B, C)
    n = 0
    for b, c, gamma, eps, wk in lh.focal_cases(shapes=[(B, C)]):
        w = lh.class_weight(wk, t, C)
        if gamma == 0.5:  # the reference itself is finite here
            assert float((1.0 - lh.focal_pt(z.double(), t, eps)).min()) > 1e-4
        check_case(lh.focal_key(B, C, gamma, eps, wk),
                   lambda red: FocalLoss(gamma=gamma, weight=w, label_smoothing=eps, reduction=red),
                   lambda x, red: lh.focal_loss(x, t, gamma, w, eps, red), z, t, cuda)
        n += 1
    assert n == (21 if C == 1 else 24)


@pytest.mark.parametrize("B,C", lh.SHAPES + [(3, 1024)], ids=lambda v: str(v))
def test_smoothed_ce_grid(cuda, B, C):
    z, t = lh.shape_inputs(B, C)
    kinds = set()
    for b, c, eps, wk, tk in lh.ce_cases(shapes=[(B, C)]):
        w, tt = lh.class_weight(wk, t, C), lh.ce_targets(tk, t)
        check_case(lh.ce_key(B, C, eps, wk, tk),
                   lambda red: SmoothedCrossEntropyLoss(weight=w, label_smoothing=eps, reduction=red),
                   lambda x, red: lh.smoothed_ce(x, tt, w, eps, lh.IGNORE, red), z, tt, cuda)
        kinds.add(tk)
    assert "plain" in kinds and ("ign" in kinds) == (B >= 4)


def test_ce_ignore_index_inside_class_range(cuda):
    """ignore_index 1 with 3 classes: those rows are ignored, not treated as class 1"""
    z, t = lh.shape_inputs(67, 3)
    w = lh.class_weight("invfreq", t, 3)
    for red in lh.REDUCTIONS:
        loss, dz = hip(SmoothedCrossEntropyLoss(weight=w, label_smoothing=0.1, ignore_index=1, reduction=red), z, t, cuda)
        ref_loss, ref_dz = lh.with_grad(lh.smoothed_ce, z.double(), t, w, 0.1, 1, red)
        close(loss, ref_loss, f"ignore 1 {red} loss")
        close(dz, ref_dz, f"ignore 1 {red} dlogits")
        assert not dz[t == 1].any()


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_focal_saturated_batch(cuda, gamma):
    """logit gap 40: pt rounds to 1 on the rows labelled with the winning class; loss and gradients stay finite and
    equal torch's (the reference's fp32 output in the golden, and the fp64 restatement)"""
    G = golden()
    z, t = G["in/sat/logits"], G["in/sat/targets"]
    key = f"focal/sat/g{gamma}"
    for red in lh.REDUCTIONS:
        loss, dz = hip(FocalLoss(gamma=gamma, reduction=red), z, t, cuda)
        assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
        close(loss, G[f"{key}/{'rows' if red == 'none' else red}"], f"{key} {red} loss")
        ref_loss, ref_dz = lh.with_grad(lh.focal_loss, z.double(), t, gamma, None, 0.0, red)
        close(loss, ref_loss, f"{key} {red} loss vs fp64")
        close(dz, ref_dz, f"{key} {red} dlogits vs fp64")
        if red == "mean":
            close(dz, G[f"{key}/dmean"], f"{key} dlogits")


@pytest.mark.parametrize("mode", ["focal", "ce"])
def test_upstream_gradient_from_device(cuda, mode):
    """(loss * s).backward() with s a device scalar, and reduction='none' under a random (B,) upstream"""
    B, C = 67, 3
    z, t = lh.shape_inputs(B, C)
    w = lh.class_weight("invfreq", t, C)
    if mode == "focal":
        crit = lambda red: FocalLoss(gamma=2.0, weight=w, label_smoothing=0.1, reduction=red)  # noqa: E731
        oracle = lambda x, red: lh.focal_loss(x, t, 2.0, w, 0.1, red)  # noqa: E731
    else:
        t = lh.ce_targets("ign", t)
        crit = lambda red: SmoothedCrossEntropyLoss(weight=w, label_smoothing=0.1, reduction=red)  # noqa: E731
        oracle = lambda x, red: lh.smoothed_ce(x, t, w, 0.1, lh.IGNORE, red)  # noqa: E731
    s = torch.tensor(-3.25, device=cuda)
    for red in ("mean", "sum"):
        zc = z.to(cuda).requires_grad_(True)
        (crit(red).to(cuda)(zc, t.to(cuda)) * s).backward()
        _, ref = lh.with_grad(oracle, z.double(), red, upstream=torch.tensor(-3.25))
        close(zc.grad, ref, f"{mode} {red} scaled")
    up = torch.randn(B, generator=torch.Generator().manual_seed(9))
    _, dz = hip(crit("none"), z, t, cuda, upstream=up)
    _, ref = lh.with_grad(oracle, z.double(), "none", upstream=up)
    close(dz, ref, f"{mode} none, per-row upstream")


@pytest.mark.parametrize("mode", ["focal", "ce"])
def test_bit_reproducible(cuda, mode):
    z, t = lh.shape_inputs(300, 2)
    w = lh.class_weight("invfreq", t, 2)
    crit = (FocalLoss(gamma=2.0, weight=w, label_smoothing=0.1) if mode == "focal" else
            SmoothedCrossEntropyLoss(weight=w, label_smoothing=0.1))
    (l1, d1), (l2, d2) = hip(crit, z, t, cuda), hip(crit, z, t, cuda)
    assert torch.equal(l1, l2) and torch.equal(d1, d2)


def test_opcheck(cuda):
    z, t = lh.shape_inputs(67, 3)
    z, targets = z.to(cuda), {"focal": t.to(cuda), "ce": lh.ce_targets("ign", t).to(cuda)}
    w = torch.tensor([0.5, 1.0, 2.0], device=cuda)
    for mode, red in (("focal", "mean"), ("ce", "mean"), ("focal", "none"), ("ce", "sum")):
        t = targets[mode]
        args = (z.clone().requires_grad_(True), t, w, mode, red, 2.0, 0.1, lh.IGNORE)
        torch.library.opcheck(torch.ops.dfd.classification_loss.default, args)
        loss, work = torch.ops.dfd.classification_loss(*args)
        torch.library.opcheck(torch.ops.dfd.classification_loss_backward.default,
                              (torch.ones_like(loss), t, w, work.detach(), 3, mode, red, 2.0, 0.1, lh.IGNORE))


@pytest.mark.parametrize("mode", ["focal", "ce"])
def test_label_guard(cuda, mode):
    """label C on one middle row and -1 on another: NaN losses and zero gradients on those rows, every other row as
    without them (in ce mode: as with those rows ignored), for every reduction's gradient.  ``weight`` is the first
    C entries of a longer tensor, so even an unguarded w[C] or w[-1] would stay inside a live allocation."""
    B, C = 67, 3
    z, t = lh.shape_inputs(B, C)
    bad = [20, 41]
    tb = t.clone()
    tb[bad[0]], tb[bad[1]] = C, -1
    good = torch.ones(B, dtype=torch.bool)
    good[bad] = False
    long_w = torch.cat([torch.full((8,), 777.0), torch.tensor([0.5, 1.0, 2.0]), torch.full((8,), 777.0)]).to(cuda)
    w = long_w[8:8 + C]  # handed to the operator as it is (the modules would copy it into their buffer)
    wc = w.cpu()

    assert w.data_ptr() == long_w.data_ptr() + 32

    def run(red):
        zc = z.to(cuda).requires_grad_(True)
        loss = torch.ops.dfd.classification_loss(zc, tb.to(cuda), w, mode, red, 2.0, 0.1, lh.IGNORE)[0]
        loss.backward(torch.ones_like(loss))
        return loss.detach().cpu(), zc.grad.cpu()

    rows, dz = run("none")
    assert torch.isnan(rows[bad]).all() and torch.isfinite(rows[good]).all()
    if mode == "focal":  # the rows that remain, as a batch of their own
        ref_rows, ref_dz = lh.with_grad(lh.focal_loss, z[good].double(), t[good], 2.0, wc, 0.1, "none")
    else:
        ti = tb.clone()
        ti[bad] = lh.IGNORE
        ref_rows, ref_dz = lh.with_grad(lh.smoothed_ce, z.double(), ti, wc, 0.1, lh.IGNORE, "none")
        ref_rows, ref_dz = ref_rows[good], ref_dz[good]
    close(rows[good], ref_rows, f"{mode} rows beside a bad label")
    close(dz[good], ref_dz, f"{mode} dlogits beside a bad label")
    assert not dz[bad].any()
    for red in ("mean", "sum"):
        loss, d = run(red)
        assert torch.isnan(loss) and not d[bad].any() and torch.isfinite(d).all()
        if mode == "focal":
            scale = 1.0 / B if red == "mean" else 1.0
            close(d[good], ref_dz * scale, f"focal {red} dlogits beside a bad label")
        else:
            _, rd = lh.with_grad(lh.smoothed_ce, z.double(), ti, wc, 0.1, lh.IGNORE, red)
            close(d[good], rd[good], f"ce {red} dlogits beside a bad label")


def test_class_count_limit(cuda):
    from deepfake_amd import _lib
    with pytest.raises(_lib.DFDError):
        FocalLoss()(torch.zeros(2, 1025, device=cuda), torch.zeros(2, dtype=torch.long, device=cuda))


# ---------------------------------------------------------------- ImprovedTrainStep
CFG = dict(learning_rate=1e-3, weight_decay=1e-2, max_epochs=10, label_smoothing=0.1, focal_gamma=2.0)
_STEP = {}


def _criterion(loss_name, cw):
    if loss_name == "focal":
        return lambda lg, y: lh.focal_loss(lg, y, CFG["focal_gamma"], cw, CFG["label_smoothing"])
    return lambda lg, y: lh.smoothed_ce(lg, y, cw, CFG["label_smoothing"])


def oracle_steps():
    """``vit_helpers.oracle_model('C')`` on the CPU in fp64 and fp32: one forward per dtype, one backward per
    criterion.  Registered with ``vit_helpers`` as cases 'C/focal' and 'C/cross_entropy' (the shapes of case C, the
    restated criterion in place of the weighted CE), so ``vit_helpers.grad_violations`` judges them unchanged."""
    if _STEP:
        return _STEP
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    x, a, labels, cw = vh.inputs("C")
    for mode, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        m = vh.oracle_model("C").to(dt)
        logits = m(x.to(dt), a.to(dt))
        params = dict(m.named_parameters())
        for loss_name in ("focal", "cross_entropy"):
            loss = _criterion(loss_name, cw.to(dt))(logits, labels)
            grads = torch.autograd.grad(loss, list(params.values()), retain_graph=True)
            run = dict(logits=logits.detach(), loss=float(loss.detach()), grads=dict(zip(params, grads)))
            vh.CASES[f"C/{loss_name}"] = vh.CASES["C"]
            vh._RUN[(f"C/{loss_name}", mode)] = run
            _STEP[(loss_name, mode)] = run
    return _STEP


@pytest.mark.parametrize("loss_name", ["focal", "cross_entropy"])
def test_improved_train_step(cuda, loss_name):
    """zero_grad, model(frames, A_norm), criterion, backward, clip 1.0 + AdamW: the loss at the project tolerance,
    every gradient element (before the optimizer) by ``vit_helpers.grad_violations``, the update against
    clip_grad_norm_(1.0) + torch AdamW applied to the same gradients, and two epochs of the cosine schedule."""
    from deepfake_amd.trainer import ImprovedTrainStep
    from deepfake_amd.vit_gcn import DeepfakeModel

    ref = oracle_steps()[(loss_name, "fp32")]
    c = vh.CASES["C"]
    x, a, labels, cw = vh.inputs("C")
    m = DeepfakeModel(gcn_hid=c["hid"], gcn_out=c["out"], num_classes=c["classes"], compute_dtype="fp32",
                      depth=c["depth"])
    m.load_state_dict(vh.oracle_model("C").state_dict())
    m.gcn.dropout.p = 0.0
    m.classifier[2].p = 0.0
    m = m.to(cuda).train()
    ts = ImprovedTrainStep(m, dict(CFG, loss=loss_name, class_weights=cw.tolist()))
    before = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    loss, logits = ts.forward_backward(x.to(cuda), a.to(cuda), labels.to(cuda))
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
    ts.optimizer.step()
    after = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    print(f"{loss_name}: loss {float(loss.detach()):.6f} (torch fp32 {ref['loss']:.6f})")
    close(logits, ref["logits"], "logits")
    assert abs(float(loss.detach()) - ref["loss"]) <= RTOL * abs(ref["loss"]) + ATOL
    bad, wt, wr, wc, wz = vh.grad_violations(grads, f"C/{loss_name}", "fp32", "cpu")
    print(f"{loss_name}: worst ratios tensor {wt:.2f}, row {wr:.2f}, column {wc:.2f}, zeros {wz:.3f}")
    assert not bad, bad[:12]
    # the optimizer on the same gradients: clip_grad_norm_(1.0) + AdamW(lr, weight_decay, betas (0.9, 0.999))
    ps = {n: torch.nn.Parameter(v.clone()) for n, v in before.items()}
    for n, p in ps.items():
        p.grad = grads[n].clone()
    opt = torch.optim.AdamW(ps.values(), lr=CFG["learning_rate"], weight_decay=CFG["weight_decay"], betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=CFG["max_epochs"], eta_min=CFG["learning_rate"] * 0.01)
    torch.nn.utils.clip_grad_norm_(ps.values(), max_norm=1.0)
    opt.step()
    for n in ps:
        close(after[n], ps[n].detach(), f"{n} after the step")
    assert max(float((after[n] - before[n]).abs().max()) for n in ps) >= 0.5 * CFG["learning_rate"]
    assert ts.optimizer.param_groups[0]["lr"] == CFG["learning_rate"]
    for _ in range(2):
        ts.scheduler_step()
        sched.step()
        assert ts.optimizer.param_groups[0]["lr"] == opt.param_groups[0]["lr"] < CFG["learning_rate"]
