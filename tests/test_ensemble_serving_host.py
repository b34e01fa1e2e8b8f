"""Serving an ensemble (CPU part): the service, the enhanced agent and the ensemble checkpoint loader against the
reference app's own outputs.

Goldens: tests/golden/make_ensemble_serving_golden.py ran ``app.predict_video`` with
``MODEL_TYPE='ensemble_pretrained'`` (``app.py:2027-2223``, the agent's step ``:2118-2171`` included), the reference
``EnhancedDecisionAgent.process_ensemble_output`` and ``app.load_model(path, 'ensemble_pretrained')``
(``app.py:1593-1679``) on the cases of tests/golden/ensemble_serving_cases.py.

* ``FrameClassifierService`` over a stub ensemble gives result dicts EQUAL to the app's, by the app's literal route
  (a stub that only has ``.models``: the forward, then every member once more) and by the decision-block route (a
  stub with ``forward_members``: every member once, ``ensemble_decide_host``, ``process_probs``);
* the agent's abstain route, temperature, class index and threshold arguments against the reference class;
* ``process_probs`` and ``process_ensemble_output`` agree; ``batch_process``; the injectable sinks;
* ``load_ensemble``: ``LAST_LOAD_STATS``, refusals, every tensor round-trips, the trainer's save format.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from ensemble_serving_cases import (AGENT_CASES, ENS_CKPT_VARIANTS, ENSEMBLE_CASES, ens_ckpt_variant,  # noqa: E402
                                    faces_for, member_scores)

from deepfake_amd import checkpoint as ck  # noqa: E402
from deepfake_amd import serving  # noqa: E402
from deepfake_amd.agent import AlertLevel, EnhancedDecisionAgent, EnsemblePrediction  # noqa: E402
from deepfake_amd.pretrained_detector import EnsembleDetector  # noqa: E402

ENV_KEYS = ("MAX_FRAMES", "MIN_FACES", "DETECT_ABSTAIN_CONF", "DETECT_ABSTAIN_MARGIN", "DETECT_FAKE_THRESHOLD",
            "ALLOW_EXTREME_CALIBRATION_THRESHOLD", "FAKE_CLASS_INDEX", "DISABLE_ENHANCED_AGENT", "ENSEMBLE_BACKBONES")
IDS = [c["name"] for c in ENSEMBLE_CASES]


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(serving, "_DEFAULT_AGENT", None)  # the app's module-level agent, fresh per case
    return monkeypatch


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "ensemble_serving_app.json")))


class StubMember(torch.nn.Module):
    def __init__(self, index, logits, raise_on_call=None):
        super().__init__()
        self.index, self.raise_on_call, self.calls = index, raise_on_call, 0
        self.logits = torch.tensor([logits], dtype=torch.float32)

    def forward(self, x):
        self.calls += 1
        if self.raise_on_call is not None and self.calls == self.raise_on_call:
            raise RuntimeError("device lost")
        b, t = x.shape[0], x.shape[1]
        return self.logits.expand(b, -1).clone(), member_scores(self.index, t).expand(b, -1).clone()


class StubEnsemble(torch.nn.Module):
    """``.models``, ``ensemble_method``, ``weights`` and this package's ``EnsembleDetector.forward``."""

    forward = EnsembleDetector.forward

    def __init__(self, case):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        roc = case.get("raise_on_call", {})
        self.models = torch.nn.ModuleList([StubMember(i, z, roc.get(str(i))) for i, z in enumerate(case["members"])])
        self.ensemble_method = case["method"]
        if "weights" in case:
            self.weights = torch.nn.Parameter(torch.tensor(case["weights"], dtype=torch.float32))


class StubEnsembleMembers(StubEnsemble):
    """the same with ``forward_members``: every member once, the combination in ``ensemble_decide`` (CPU: host)"""

    def forward_members(self, x, fake_idx=1, temperature=1.0, return_block=False):
        outs = [m(x) for m in self.models]
        zl, zs = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        out = serving.ensemble_decide(zl, zs, getattr(self, "weights", None), self.ensemble_method, fake_idx,
                                      temperature)
        return (out[0], out[1], zl, zs, out[2]) if return_block else (out[0], out[1], zl, zs)


def _service(case, clean_env, tmp_path, cls):
    for k, v in case.get("env", {}).items():
        clean_env.setenv(k, v)
    if "calibration" in case:
        (tmp_path / "calibration_best.json").write_text(json.dumps(case["calibration"]))
    model = cls(case)
    return model, serving.FrameClassifierService(model, checkpoint_path=str(tmp_path / "checkpoint_best.pt"),
                                                 device="cpu")


@pytest.mark.parametrize("case", ENSEMBLE_CASES, ids=IDS)
def test_literal_route_matches_reference_app(case, clean_env, tmp_path, gold):
    g = {r["name"]: r for r in gold["cases"]}[case["name"]]
    model, svc = _service(case, clean_env, tmp_path, StubEnsemble)
    res = svc.predict_video(str(tmp_path / "clip.mp4"), lambda path, max_frames=16: faces_for(case))
    assert res == g["result"]
    assert [m.calls for m in model.models] == g["member_calls"]  # the app's two passes per member


@pytest.mark.parametrize("case", ENSEMBLE_CASES, ids=IDS)
def test_block_route_matches_reference_app(case, clean_env, tmp_path, gold):
    """One pass per member and the decision block give the app's result dict; a member that fails on a second
    call is never called twice (its case then equals the same case without the failure)."""
    g = {r["name"]: r for r in gold["cases"]}
    exp = g[case["name"]]["result"]
    if case["name"] == "member_raises_second":
        exp = g["avg_agree_fake"]["result"]
    model, svc = _service(case, clean_env, tmp_path, StubEnsembleMembers)
    res = svc.predict_video(str(tmp_path / "clip.mp4"), lambda path, max_frames=16: faces_for(case))
    assert res == exp
    assert all(m.calls <= 1 for m in model.models)


def test_case_coverage(gold):
    by = {c["name"]: c for c in ENSEMBLE_CASES}
    res = {r["name"]: r["result"] for r in gold["cases"]}
    assert {c["method"] for c in ENSEMBLE_CASES} == {"average", "weighted", "voting"}
    assert {len(c["members"]) for c in ENSEMBLE_CASES} >= {1, 2, 3}
    for env in ("FAKE_CLASS_INDEX", "DISABLE_ENHANCED_AGENT", "DETECT_ABSTAIN_MARGIN", "DETECT_ABSTAIN_CONF"):
        assert any(env in c.get("env", {}) for c in ENSEMBLE_CASES), env
    # the M = 2 voting tie goes to class 0: one-hot [1, 0]
    assert by["voting_tie_m2"]["method"] == "voting" and res["voting_tie_m2"]["prob_fake"] == pytest.approx(
        1.0 / (1.0 + np.e), abs=1e-6)
    # the agent's decision threshold follows the calibration file: fake below 0.5
    assert res["calib_thr"]["threshold"] == 0.3 and res["calib_thr"]["prob_fake"] < 0.5
    assert res["calib_thr"]["enhanced_agent"]["is_fake"] is True
    # the agent's confidence, not the plain one, meets the abstain rules
    assert res["abstain_conf_low"]["abstained"] and res["abstain_conf_low"]["confidence"] < 0.05
    assert res["margin"]["abstained"] and res["margin"]["description"].startswith("Borderline")
    assert res["member_raises_second"]["enhanced_agent"] is None and res["member_raises_second"]["pred_class"] == 1
    assert res["agent_disabled"]["enhanced_agent"] is None
    # an adjusted probability just either side of the threshold, and on it (plain rule: fake; agent: not)
    assert res["adjusted_above_thr"]["pred_class"] == 1 and res["adjusted_below_thr"]["pred_class"] == 0
    assert res["adjusted_at_thr"]["prob_fake"] == 0.5 and res["adjusted_at_thr"]["pred_class"] == 0


def test_batch_matches_single(clean_env):
    cases = [c for c in ENSEMBLE_CASES if c["method"] == "average" and len(c["members"]) == 2
             and not c.get("env") and "calibration" not in c and "raise_on_call" not in c]
    for cls in (StubEnsemble, StubEnsembleMembers):
        svc = serving.FrameClassifierService(cls(cases[0]), device="cpu")
        faces = [faces_for(c) for c in cases] + [faces_for(cases[0])[:0]]
        assert svc.predict_batch(faces) == [svc.predict_faces(f) for f in faces]


def test_decide_without_agent_inputs_is_unchanged(clean_env):
    row = torch.tensor([-1.0, 1.5])
    plain = serving.decide(row, 4, ensemble=True)
    assert plain["enhanced_agent"] is None and plain["description"] == "Ensemble pretrained detector (thr=0.50)"
    assert serving.decide(row, 4, None, None, True) == plain


def test_decide_restores_threshold_and_sets_class_index(clean_env):
    agent = EnhancedDecisionAgent(decision_threshold=0.42)
    clean_env.setenv("DETECT_FAKE_THRESHOLD", "0.7")
    clean_env.setenv("FAKE_CLASS_INDEX", "0")
    z = [torch.tensor([2.0, -1.0]), torch.tensor([1.5, -0.5])]
    res = serving.decide(torch.stack(z).mean(0), 4, ensemble=True, agent=agent, video_id="a.mp4",
                         agent_inputs={"individual_logits": z, "frame_scores": None})
    assert res["enhanced_agent"] is not None and res["threshold"] == 0.7
    assert agent.decision_threshold == 0.42 and agent.fake_class_index == 0


# ------------------------------------------------------------------------------ the agent on its own
def _fields(pred):
    return {"video_id": pred.video_id, "is_fake": None if pred.is_fake is None else bool(pred.is_fake),
            "confidence": float(pred.confidence), "alert_level": pred.alert_level.name,
            "ensemble_prob": float(pred.ensemble_prob), "individual_probs": [float(p) for p in pred.individual_probs],
            "uncertainty": float(pred.uncertainty), "explanation": str(pred.explanation)}


def _agent_call(case):
    agent = EnhancedDecisionAgent(**case.get("kwargs", {}))
    ens = torch.tensor([case["ensemble"]], dtype=torch.float32)
    ind = [torch.tensor(z, dtype=torch.float32) for z in case["individual"]]
    return agent, ens, ind


@pytest.mark.parametrize("case", AGENT_CASES, ids=[c["name"] for c in AGENT_CASES])
def test_agent_matches_reference_class(case, gold):
    g = {r["name"]: r for r in gold["agent"]}[case["name"]]
    agent, ens, ind = _agent_call(case)
    pred = agent.process_ensemble_output(ens, ind, member_scores(0, 4).unsqueeze(0), case["name"] + ".mp4",
                                         uncertainty=case["uncertainty"])
    assert isinstance(pred, EnsemblePrediction) and isinstance(pred.alert_level, AlertLevel)
    assert {"name": case["name"], **_fields(pred)} == g
    assert np.array_equal(pred.frame_scores, member_scores(0, 4).numpy())


def test_agent_abstain_route_is_covered(gold):
    g = {r["name"]: r for r in gold["agent"]}
    assert g["abstain"]["is_fake"] is None and g["abstain"]["explanation"].startswith("Abstained")
    assert g["abstain_switched_off"]["is_fake"] is not None


@pytest.mark.parametrize("case", AGENT_CASES, ids=[c["name"] for c in AGENT_CASES])
def test_agent_entry_points_agree(case):
    agent, ens, ind = _agent_call(case)
    a = agent.process_ensemble_output(ens, ind, member_scores(0, 4), "v", uncertainty=case["uncertainty"])
    idx, temp = agent.fake_index(), agent.temperature
    fake_prob = torch.softmax(ens / temp, dim=1)[0, idx].item()
    probs = [torch.softmax(z.unsqueeze(0) / temp, dim=1)[0, idx].item() for z in ind]
    b = agent.process_probs(fake_prob, probs, member_scores(0, 4), "v", uncertainty=case["uncertainty"])
    assert _fields(a) == _fields(b)
    # ... and with the values of a decision block
    _, _, block = serving.ensemble_decide_host(torch.stack(ind).unsqueeze(1), torch.zeros(len(ind), 1, 4), None,
                                               "average", idx, temp)
    inputs = serving.block_agent_inputs(block[0].tolist())
    c = agent.process_probs(fake_prob, inputs["individual_probs"], member_scores(0, 4), "v",
                            uncertainty=case["uncertainty"])
    assert _fields(a) == _fields(c)


def test_agent_batch_process_and_sinks():
    class Sink:
        def __init__(self):
            self.events = []

        def log_event(self, e):
            self.events.append(e)

        def queue_for_label(self, e):
            self.events.append({"queued": True, **e})

    agent = EnhancedDecisionAgent()
    assert agent.telemetry is None and agent.active_learner is None and agent.queue_low_confidence_below == 0.05
    agent.telemetry, agent.active_learner = Sink(), Sink()
    ens = torch.tensor([[-1.0, 2.0], [0.0, 0.0]])
    ind = [torch.tensor([[-1.0, 1.5], [6.0, -6.0]]), torch.tensor([[-0.5, 2.0], [-6.0, 6.0]])]
    out = agent.batch_process(ens, ind, torch.full((2, 4), 0.25), ["a", "b"], uncertainties=torch.tensor([0.0, 0.8]))
    one = [agent.process_ensemble_output(ens[i], [z[i] for z in ind], torch.full((4,), 0.25), v, u)
           for i, (v, u) in enumerate((("a", 0.0), ("b", float(torch.tensor(0.8)))))]
    assert [_fields(p) for p in out] == [_fields(p) for p in one]
    assert out[0].is_fake is True and out[1].is_fake is None
    assert [e["event"] for e in agent.telemetry.events] == ["decision", "abstain"] * 2
    assert [e["video_id"] for e in agent.active_learner.events] == ["b", "b"]  # the abstained video is queued

    class Broken:
        def log_event(self, e):
            raise OSError("disk full")

    agent.telemetry = Broken()  # a failing sink never costs the decision
    assert agent.process_ensemble_output(ens[0], [z[0] for z in ind], torch.zeros(4), "a").is_fake is True


# ------------------------------------------------------------------------------ ensemble_decide_host
def test_host_contract_is_the_ensemble_forward():
    case = {"method": "weighted", "weights": [0.3, -0.2], "members": [[-1.0, 2.0], [0.5, 1.0]]}
    x = torch.zeros(3, 5, 3, 8, 8)
    for method in ("average", "weighted", "voting"):
        model = StubEnsembleMembers({**case, "method": method})
        logits, scores = model(x)
        hl, hs, zl, zs, block = model.forward_members(x, fake_idx=0, temperature=1.7, return_block=True)
        assert torch.equal(hl, logits) and torch.equal(hs, scores)
        assert zl.shape == (2, 3, 2) and zs.shape == (2, 3, 5) and block.shape == (3, 9)
        assert torch.equal(block[:, 4], torch.full((3,), 2.0))
        assert torch.equal(block[:, 0], torch.softmax(logits, 1)[:, 0])
        assert torch.equal(block[:, 1], torch.softmax(logits, 1)[:, 1])
        assert torch.equal(block[:, 2], torch.softmax(logits / 1.7, 1)[:, 0])
        assert torch.equal(block[:, 5:7], torch.softmax(zl, 2)[:, :, 0].T)
        assert torch.equal(block[:, 7:9], torch.softmax(zl / 1.7, 2)[:, :, 0].T)
    for bad in (dict(method="median"), dict(fake_idx=2), dict(temperature=0.0)):
        kw = {"method": "average", "fake_idx": 1, "temperature": 1.0, **bad}
        with pytest.raises(ValueError):
            serving.ensemble_decide_host(torch.zeros(2, 1, 2), torch.zeros(2, 1, 4), None, **kw)
    with pytest.raises(ValueError):
        serving.ensemble_decide_host(torch.zeros(2, 1, 2), torch.zeros(2, 1, 4), None, "weighted", 1, 1.0)
    with pytest.raises(ValueError):
        serving.ensemble_decide_host(torch.zeros(9, 1, 2), torch.zeros(9, 1, 4), None, "average", 1, 1.0)


def test_forward_members_refuses_training_mode_and_cpu():
    ens = EnsembleDetector(["efficientnet_b0"], pretrained=False)
    with pytest.raises(RuntimeError, match="eval"):
        ens.train().forward_members(torch.zeros(1, 2, 3, 64, 64))
    with pytest.raises(RuntimeError):  # no CPU fallback for the HIP members
        ens.eval().forward_members(torch.zeros(1, 2, 3, 64, 64))


# ------------------------------------------------------------------------------ load_ensemble
@pytest.fixture(scope="module")
def load_gold():
    return {r["name"]: r for r in json.load(open(os.path.join(HERE, "golden", "ensemble_load.json")))["loads"]}


@pytest.mark.parametrize("name", ENS_CKPT_VARIANTS)
def test_load_ensemble_matches_reference_app(name, tmp_path, load_gold, monkeypatch):
    monkeypatch.delenv("ENSEMBLE_BACKBONES", raising=False)
    g = load_gold[name]
    obj = ens_ckpt_variant(name)
    p = tmp_path / "checkpoint_best.pt"
    torch.save(obj, p)
    if not g["ok"]:
        with pytest.raises(ck.IncompatibleCheckpoint, match="match_ratio"):
            ck.load_ensemble(p)
        return
    model, stats = ck.load_ensemble(p)
    assert stats == g["stats"]
    assert isinstance(model, EnsembleDetector) and model.ensemble_method == g["ensemble_method"] == "weighted"
    assert not model.training
    sd = ck.normalize_state_dict_keys(ck.extract_state_dict(obj))
    msd = model.state_dict()
    assert set(sd) == set(msd)
    for k, v in sd.items():  # every tensor round-trips
        assert torch.equal(msd[k].cpu(), v), k


def test_load_ensemble_candidates_and_refusals(tmp_path, monkeypatch):
    monkeypatch.delenv("ENSEMBLE_BACKBONES", raising=False)
    assert ck.infer_ensemble_count({"models.0.fc1.bias": 0, "models.2.x": 0, "weights": 0}) == 3
    assert ck.infer_ensemble_count({"fc1.bias": 0}) is None
    assert ck.ensemble_candidates(["efficientnet_b0", "resnet50"], 2)[0] == ["efficientnet_b0", "resnet50"]
    assert ck.ensemble_candidates(["resnet50", "efficientnet_b0"], 2)[0] == ["resnet50", "efficientnet_b0"]
    assert ck.ensemble_candidates(["efficientnet_b0", "resnet50"], 1)[:2] == [["efficientnet_b0"], ["resnet50"]]
    assert ck.ensemble_candidates(["efficientnet_b0"], 4) == [["efficientnet_b0", "resnet50", "resnet34", "resnet18"]]
    with pytest.raises(ck.IncompatibleCheckpoint, match="No state_dict"):
        ck.load_ensemble({})
    # three members: every list the app would try names a backbone without a HIP trunk
    sd3 = {f"models.{i}.fc2.bias": torch.zeros(2) for i in range(3)}
    with pytest.raises(ck.IncompatibleCheckpoint, match="3 member"):
        ck.load_ensemble(sd3)
    # the requested order is tried first and wins when it fits: resnet50 first
    swapped = ens_ckpt_variant("swapped_members")
    model, stats = ck.load_ensemble(swapped, meta={"backbones": ["resnet50", "efficientnet_b0"]})
    assert stats["backbones"] == ["resnet50", "efficientnet_b0"] and stats["match_ratio"] == 1.0
    monkeypatch.setenv("ENSEMBLE_BACKBONES", "resnet50, efficientnet_b0")
    assert ck.load_ensemble(swapped)[1]["backbones"] == ["resnet50", "efficientnet_b0"]


def test_trainer_checkpoint_loads_into_the_service(tmp_path, monkeypatch):
    """``EnsembleTrainer._save_checkpoint`` writes ``checkpoint.save_state_dict(model, 'checkpoint_best.pt')``: that
    file loads with every key matched, and ``FrameClassifierService.from_checkpoint`` routes it to ``load_ensemble``
    (a single detector's checkpoint still goes to ``load_pretrained``)."""
    from deepfake_amd.weights import deterministic_init_

    monkeypatch.delenv("ENSEMBLE_BACKBONES", raising=False)
    ens = EnsembleDetector(["efficientnet_b0", "resnet50"], pretrained=False, ensemble_method="weighted")
    deterministic_init_(ens, seed=3)
    p = tmp_path / "checkpoint_best.pt"
    ck.save_state_dict(ens, p)
    model, stats = ck.load_ensemble(p)
    assert stats["match_ratio"] == 1.0 and stats["missing"] == 0 and stats["unexpected"] == 0
    for k, v in ens.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    svc = serving.FrameClassifierService.from_checkpoint(p, device="cpu")
    assert isinstance(svc.model, EnsembleDetector) and svc.load_stats["model_type"] == "ensemble_pretrained"
    assert svc.load_stats["checkpoint"] == str(p)
    # an 'average' ensemble saves no `weights`: one key of the weighted model is missing, the rest match
    avg = EnsembleDetector(["efficientnet_b0", "resnet50"], pretrained=False, ensemble_method="average")
    ck.save_state_dict(avg, p)
    _, stats = ck.load_ensemble(p)
    assert stats["missing"] == 1 and stats["matched"] == stats["model_keys"] - 1
    single = tmp_path / "checkpoint_best_efficientnet_b0.pt"
    ck.save_state_dict(ens.models[0], single)
    svc = serving.FrameClassifierService.from_checkpoint(single, device="cpu")
    assert not hasattr(svc.model, "models") and svc.load_stats["model_type"] == "pretrained"
