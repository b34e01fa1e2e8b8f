"""Case definitions shared by tests/golden/make_ensemble_serving_golden.py (which runs the reference app and the
reference's EnhancedDecisionAgent on them) and tests/test_ensemble_serving_host.py / test_ensemble_decide_gpu.py
(which run this package on them).  Data only: stub member logits, ensemble methods and weights, environment
settings, calibration files, agent arguments and ensemble checkpoint layouts; plus the CPU oracle members the
checkpoints are written from."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from deepfake_amd.weights import deterministic_init_

# members: one [class 0, class 1] logit pair per stub member; n: face crops (= frames T); weights: the raw
# ensemble weight vector of a 'weighted' ensemble; raise_on_call: {member index: the call (1-based) that raises}
ENSEMBLE_CASES = [
    {"name": "avg_agree_fake", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]]},
    {"name": "avg_agree_real", "method": "average", "members": [[2.0, -1.0], [1.5, -0.5]], "n": 8},
    {"name": "avg_disagree", "method": "average", "members": [[2.0, -1.0], [-1.0, 2.5]]},
    {"name": "avg_m3", "method": "average", "members": [[-2.0, 2.0], [-1.0, 3.0], [0.5, 1.5]], "n": 3},
    {"name": "weighted_m2", "method": "weighted", "weights": [0.3, -0.2], "members": [[-1.0, 2.0], [0.5, 1.0]]},
    {"name": "weighted_m3", "method": "weighted", "weights": [0.1, 0.5, -0.4],
     "members": [[1.0, -2.0], [2.5, -0.5], [-0.5, 0.25]], "n": 5},
    {"name": "weighted_m1", "method": "weighted", "weights": [0.7], "members": [[-0.5, 1.5]]},
    {"name": "voting_tie_m2", "method": "voting", "members": [[2.0, -1.0], [-1.0, 2.0]]},
    {"name": "voting_m2_fake", "method": "voting", "members": [[-2.0, 1.0], [-1.0, 2.0]]},
    {"name": "voting_m3_fake", "method": "voting", "members": [[2.0, -1.0], [-1.0, 2.0], [-0.5, 0.5]], "n": 6},
    {"name": "voting_m3_argmax_tie", "method": "voting", "members": [[0.5, 0.5], [-1.0, 2.0], [1.0, 1.0]]},
    {"name": "voting_m1", "method": "voting", "members": [[-1.0, 2.0]]},
    {"name": "avg_m1", "method": "average", "members": [[-0.5, 1.5]]},
    {"name": "calib_thr", "method": "average", "members": [[0.3, 0.0], [0.6, 0.1]],
     "calibration": {"best_thr_accuracy": 0.3}, "env": {"DETECT_ABSTAIN_CONF": "0.05"}},
    {"name": "thr_env_high", "method": "average", "members": [[-1.0, 0.5], [-0.8, 0.4]],
     "env": {"DETECT_FAKE_THRESHOLD": "0.9", "DETECT_ABSTAIN_CONF": "0.0"}},
    {"name": "fake_idx0", "method": "average", "members": [[2.0, -1.0], [1.5, -0.5]],
     "env": {"FAKE_CLASS_INDEX": "0"}},
    {"name": "fake_idx0_weighted", "method": "weighted", "weights": [-0.5, 0.5],
     "members": [[-2.0, 1.0], [-1.5, 2.5]], "env": {"FAKE_CLASS_INDEX": "0"}},
    {"name": "agent_disabled", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "env": {"DISABLE_ENHANCED_AGENT": "1"}},
    {"name": "agent_disabled_true", "method": "voting", "members": [[2.0, -1.0], [-1.0, 2.0]],
     "env": {"DISABLE_ENHANCED_AGENT": "true"}},
    {"name": "margin", "method": "average", "members": [[0.0, 0.3], [0.1, 0.2]],
     "env": {"DETECT_ABSTAIN_MARGIN": "0.1"}},
    {"name": "margin_outside", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "env": {"DETECT_ABSTAIN_MARGIN": "0.1"}},
    {"name": "abstain_conf_low", "method": "average", "members": [[2.0, -1.0], [-1.0, 2.5]],
     "env": {"DETECT_ABSTAIN_CONF": "0.05"}},
    {"name": "abstain_conf_high", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "env": {"DETECT_ABSTAIN_CONF": "0.9"}},
    {"name": "member_raises_second", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "raise_on_call": {"1": 2}},
    {"name": "member_raises_first", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "raise_on_call": {"0": 1}},
    {"name": "adjusted_above_thr", "method": "average", "members": [[0.0, 0.0004]],
     "env": {"DETECT_ABSTAIN_CONF": "0.0"}},
    {"name": "adjusted_below_thr", "method": "average", "members": [[0.0, -0.0004]],
     "env": {"DETECT_ABSTAIN_CONF": "0.0"}},
    {"name": "adjusted_at_thr", "method": "average", "members": [[0.0, 0.0]], "env": {"DETECT_ABSTAIN_CONF": "0.0"}},
    {"name": "avg_disagree_strong", "method": "average", "members": [[-3.0, 3.0], [0.95, -0.95]],
     "env": {"DETECT_ABSTAIN_CONF": "0.0"}},
    {"name": "saturated", "method": "average", "members": [[-80.0, 80.0], [-80.0, 80.0]]},
    {"name": "one_face", "method": "average", "members": [[-1.0, 1.5], [-0.5, 2.0]], "n": 1},
    {"name": "one_face_min1", "method": "weighted", "weights": [0.0, 0.0], "members": [[-1.0, 1.5], [-0.5, 2.0]],
     "n": 1, "env": {"MIN_FACES": "1"}},
]

# EnhancedDecisionAgent.process_ensemble_output called directly (the app's uncertainty is a standard deviation of
# probabilities, at most 0.5: the agent's own abstain route needs an explicit one).  kwargs: constructor arguments.
AGENT_CASES = [
    {"name": "abstain", "ensemble": [0.0, 0.0], "individual": [[6.0, -6.0], [-6.0, 6.0]], "uncertainty": 0.8},
    {"name": "abstain_m3", "ensemble": [0.5, 1.0], "individual": [[5.0, -5.0], [-5.0, 5.0], [-4.0, 6.0]],
     "uncertainty": 0.95},
    {"name": "high_uncertainty_agreeing", "ensemble": [-1.0, 2.0], "individual": [[-1.0, 1.5], [-0.5, 2.0]],
     "uncertainty": 0.7},
    {"name": "high_uncertainty_low_conf", "ensemble": [0.0, 0.25], "individual": [[0.0, 0.2], [0.1, 0.2]],
     "uncertainty": 0.9},
    {"name": "abstain_switched_off", "ensemble": [0.0, 0.0], "individual": [[6.0, -6.0], [-6.0, 6.0]],
     "uncertainty": 0.8, "kwargs": {"abstain_on_high_uncertainty": False}},
    {"name": "temperature", "ensemble": [-1.0, 2.0], "individual": [[-1.0, 1.5], [-0.5, 2.0]], "uncertainty": 0.1,
     "kwargs": {"temperature": 1.7}},
    {"name": "fake_index0", "ensemble": [2.0, -1.0], "individual": [[1.0, -1.5], [0.5, -2.0]], "uncertainty": 0.0,
     "kwargs": {"fake_class_index": 0}},
    {"name": "fake_index_bad", "ensemble": [2.0, -1.0], "individual": [[1.0, -1.5], [0.5, -2.0]],
     "uncertainty": 0.0, "kwargs": {"fake_class_index": 7}},
    {"name": "custom_thresholds", "ensemble": [-0.2, 0.4], "individual": [[-0.2, 0.3], [0.0, 0.5]],
     "uncertainty": 0.2,
     "kwargs": {"confidence_thresholds": {"safe_max": 0.1, "warning_max": 0.5, "danger_max": 0.6,
                                          "critical_min": 0.6},
                "uncertainty_penalty": 0.3, "decision_threshold": 0.4}},
    {"name": "critical", "ensemble": [-4.0, 4.0], "individual": [[-4.0, 4.0], [-3.5, 4.5]], "uncertainty": 0.0},
    {"name": "safe", "ensemble": [3.0, -3.0], "individual": [[3.0, -3.0], [2.0, -2.0]], "uncertainty": 0.05},
    {"name": "one_member", "ensemble": [-0.5, 0.5], "individual": [[-0.5, 0.5]], "uncertainty": 0.0},
]


def member_scores(m: int, t: int) -> torch.Tensor:
    """frame scores (T) of stub member ``m``: a softmax over the frames, different per member"""
    return torch.softmax(torch.arange(t, dtype=torch.float32) * (0.25 * (m + 1)), dim=0)


def faces_for(case, size=16):
    from serving_cases import faces_for as _faces

    return _faces({"name": "ens/" + case["name"], "n": case.get("n", 4)}, size)


# ------------------------------------------------------------------------------ checkpoints
ENS_CKPT_SEED = 57
ENS_WEIGHTS = (0.3, -0.2)
ENS_CKPT_VARIANTS = ["raw", "module_prefix", "one_member", "swapped_members", "partial"]


class ResNetDetectorCPU(nn.Module):
    """``PretrainedBackboneDetector('resnet50')`` (src/pretrained_detector.py:37-40, 64-76, 103-143) over the
    oracle's torchvision restatement: the same head as ``oracle.detector_cpu.DetectorCPU`` on 2048 features."""

    def __init__(self, num_classes=2, dropout_rate=0.5):
        super().__init__()
        from oracle.resnet_cpu import FEATURE_DIM, ResNet50TrunkCPU

        self.backbone = ResNet50TrunkCPU()
        self.temporal_attention = nn.Sequential(nn.Linear(FEATURE_DIM, 64), nn.ReLU(), nn.Linear(64, 1), nn.Sigmoid())
        self.dropout = nn.Dropout(dropout_rate)
        self.fc1 = nn.Linear(FEATURE_DIM, 256)
        self.fc2 = nn.Linear(256, num_classes)

    def forward(self, x):
        b, t, c, h, w = x.shape
        f = self.backbone(x.reshape(b * t, c, h, w)).view(b, t, -1)
        a = F.softmax(self.temporal_attention(f).squeeze(-1), dim=1)
        g = (f * a.unsqueeze(-1)).sum(dim=1)
        return self.fc2(self.dropout(F.relu(self.fc1(self.dropout(g))))), a


def oracle_members(backbones=("efficientnet_b0", "resnet50"), seed=ENS_CKPT_SEED):
    """CPU oracle members with the portable weights, named as the ensemble's state_dict names them."""
    from oracle.detector_cpu import DetectorCPU

    out = []
    for i, name in enumerate(backbones):
        m = DetectorCPU(dropout_rate=0.5) if name == "efficientnet_b0" else ResNetDetectorCPU(dropout_rate=0.5)
        deterministic_init_(m, seed=seed, prefix=f"models.{i}.")
        out.append(m.eval())
    return out


def ensemble_state_dict(backbones=("efficientnet_b0", "resnet50"), weights=ENS_WEIGHTS):
    """The state_dict ``EnsembleDetector(backbones, ensemble_method='weighted')`` saves: ``models.<i>.*`` and
    ``weights`` (the format of ``EnsembleTrainer._save_checkpoint``, src/ensemble_trainer.py:549-571)."""
    sd = {"weights": torch.tensor(list(weights), dtype=torch.float32)}
    for i, m in enumerate(oracle_members(backbones)):
        for k, v in m.state_dict().items():
            sd[f"models.{i}.{k}"] = v.clone()
    return sd


def ens_ckpt_variant(name):
    """The checkpoint object of one layout (what torch.save writes to disk)."""
    if name == "raw":
        return ensemble_state_dict()
    if name == "module_prefix":  # DataParallel keys inside the trainer's dict format, with a class map
        return {"model_state": {"module." + k: v for k, v in ensemble_state_dict().items()},
                "class_to_idx": {"fake": 0, "real": 1}}
    if name == "one_member":
        return ensemble_state_dict(("efficientnet_b0",), (0.7,))
    if name == "swapped_members":  # resnet50 first: every trunk key and fc1 / attention shapes miss -> refused
        return ensemble_state_dict(("resnet50", "efficientnet_b0"))
    if name == "partial":  # < 80 % of the model's keys -> refused
        sd = ensemble_state_dict()
        return {k: sd[k] for i, k in enumerate(sorted(sd)) if i % 3 != 0}
    raise KeyError(name)
