"""The enhanced decision agent of the app's ensemble branch (``src/enhanced_decision_agent.py:17-346``).

``app.predict_video`` hands an ensemble's logits to ``EnhancedDecisionAgent.process_ensemble_output``
(``app.py:2118-2171``) and takes ``pred_class``, ``confidence`` and ``description`` from its answer.  This module
restates that class with the reference's constructor arguments, attributes and arithmetic, split in two:

* ``process_ensemble_output`` takes logits, as in the reference: it makes the fp32 softmaxes
  (``logits / temperature``) and hands their values on;
* ``process_probs`` takes those fp32 values -- the ensemble's fake-class probability and one per member, which is
  what ``dfd::ensemble_decide`` writes into its decision block -- and does everything the reference does in Python
  floats (double) after ``.item()``: ``np.std`` / ``np.mean``, the adjusted probability, both decision routes,
  the alert level and the formatted explanation.

Quirks kept because the app's result dicts show them: an abstaining agent reports the ADJUSTED probability as
``ensemble_prob`` and a deciding one the raw fake probability; the explanation prints the raw fake probability while
the alert level is chosen from the adjusted one; ``is_fake`` is ``None`` on the abstain route.
``DecisionAggregator`` is not restated: the app never calls it.  ``telemetry`` (``log_event(dict)``) and
``active_learner`` (``queue_for_label(dict)``) are injectable attributes, ``None`` by default; their failures are
swallowed as in the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F


class AlertLevel(Enum):
    SAFE = 0
    WARNING = 1
    DANGER = 2
    CRITICAL = 3


ALERT_NAMES = {AlertLevel.SAFE: "AUTHENTIC", AlertLevel.WARNING: "UNCERTAIN", AlertLevel.DANGER: "LIKELY DEEPFAKE",
               AlertLevel.CRITICAL: "VERY LIKELY DEEPFAKE"}


@dataclass
class EnsemblePrediction:
    video_id: str
    is_fake: Optional[bool]
    confidence: float
    alert_level: AlertLevel
    ensemble_prob: float
    individual_probs: list
    frame_scores: object  # np.ndarray, or None where the caller passed no frame scores
    uncertainty: float
    explanation: str


def _to_numpy(frame_scores):
    return frame_scores.cpu().numpy() if hasattr(frame_scores, "cpu") else frame_scores


class EnhancedDecisionAgent:
    def __init__(self, temperature: float = 1.0, confidence_thresholds: Optional[Dict] = None,
                 uncertainty_penalty: float = 0.1, fake_class_index: int = 1,
                 abstain_on_high_uncertainty: bool = True, abstain_uncertainty_threshold: float = 0.6,
                 min_agreement_to_act: float = 0.6, decision_threshold: float = 0.5):
        self.temperature = temperature
        self.uncertainty_penalty = uncertainty_penalty
        self.abstain_on_high_uncertainty = abstain_on_high_uncertainty
        self.abstain_uncertainty_threshold = abstain_uncertainty_threshold
        self.min_agreement_to_act = min_agreement_to_act
        self.decision_threshold = decision_threshold
        try:
            self.fake_class_index = int(fake_class_index)
        except Exception:
            self.fake_class_index = 1
        self.telemetry = None
        self.active_learner = None
        self.queue_low_confidence_below = 0.05
        self.thresholds = confidence_thresholds or {"safe_max": 0.30, "warning_max": 0.70, "danger_max": 0.95,
                                                    "critical_min": 0.95}

    # ------------------------------------------------------------------ entry points
    def fake_index(self) -> int:
        """``fake_class_index`` as the reference reads it: anything but 0 / 1 means 1."""
        try:
            idx = int(self.fake_class_index)
        except Exception:
            idx = 1
        return idx if idx in (0, 1) else 1

    def process_ensemble_output(self, ensemble_logits: torch.Tensor, individual_logits: list,
                                frame_scores: torch.Tensor, video_id: str,
                                uncertainty: float = 0.0) -> EnsemblePrediction:
        """ensemble_logits (C) or (1, C), individual_logits a list of (C) or (1, C), frame_scores (T) or (1, T)."""
        if ensemble_logits.dim() == 1:
            ensemble_logits = ensemble_logits.unsqueeze(0)
        if frame_scores is not None and hasattr(frame_scores, "dim") and frame_scores.dim() > 1:
            frame_scores = frame_scores.squeeze()
        idx = self.fake_index()
        fake_prob = F.softmax(ensemble_logits / self.temperature, dim=1)[0][idx].item()
        individual_probs = []
        for z in individual_logits:
            if z.dim() == 1:
                z = z.unsqueeze(0)
            individual_probs.append(F.softmax(z / self.temperature, dim=1)[0][idx].item())
        return self.process_probs(fake_prob, individual_probs, frame_scores, video_id, uncertainty)

    def process_probs(self, fake_prob: float, individual_probs: Sequence[float], frame_scores=None,
                      video_id: str = "", uncertainty: float = 0.0) -> EnsemblePrediction:
        """The decision from the fp32 fake-class probabilities at ``logits / temperature`` (as Python floats): the
        ensemble's and each member's.  Double arithmetic from here on, as the reference after ``.item()``."""
        individual_probs = list(individual_probs)
        try:
            arr = np.array(individual_probs, dtype=float)
            agreement = float(1.0 - np.std(arr))
            mean_individual = float(np.mean(arr))
        except Exception:
            agreement, mean_individual = 1.0, fake_prob
        adjusted = (0.7 * fake_prob + 0.3 * mean_individual) * (1.0 - self.uncertainty_penalty * uncertainty)

        if (self.abstain_on_high_uncertainty and uncertainty > self.abstain_uncertainty_threshold
                and agreement < self.min_agreement_to_act):
            confidence = max(0.0, (1.0 - uncertainty) * agreement)
            record = {"video_id": video_id, "ensemble_prob": adjusted, "confidence": confidence,
                      "uncertainty": uncertainty}
            self._log({"event": "abstain", **record})
            self._queue(record)
            return EnsemblePrediction(
                video_id=video_id, is_fake=None, confidence=confidence, alert_level=AlertLevel.WARNING,
                ensemble_prob=adjusted, individual_probs=individual_probs, frame_scores=_to_numpy(frame_scores),
                uncertainty=uncertainty,
                explanation=(f"Abstained: high uncertainty ({uncertainty:.2f}) and low model agreement "
                             f"({agreement:.2f})."))

        is_fake = adjusted > self.decision_threshold
        confidence = abs(adjusted - self.decision_threshold) * 2.0
        confidence = confidence * max(0.0, agreement) * (1.0 - self.uncertainty_penalty * uncertainty)
        alert = self._determine_alert_level(adjusted, confidence, uncertainty)
        explanation = self._generate_explanation(fake_prob, confidence, uncertainty, alert, individual_probs)
        record = {"video_id": video_id, "ensemble_prob": adjusted, "confidence": confidence,
                  "uncertainty": uncertainty}
        self._log({"event": "decision", "video_id": video_id, "is_fake": bool(is_fake), "ensemble_prob": adjusted,
                   "confidence": confidence, "uncertainty": uncertainty, "alert_level": alert.name})
        if confidence < self.queue_low_confidence_below:
            self._queue(record)
        return EnsemblePrediction(video_id=video_id, is_fake=is_fake, confidence=confidence, alert_level=alert,
                                  ensemble_prob=fake_prob, individual_probs=individual_probs,
                                  frame_scores=_to_numpy(frame_scores), uncertainty=uncertainty,
                                  explanation=explanation)

    def batch_process(self, ensemble_logits: torch.Tensor, individual_logits_list: list, frame_scores: torch.Tensor,
                      video_ids: list, uncertainties: Optional[torch.Tensor] = None) -> list:
        """ensemble_logits (B, C), individual_logits_list a list over members of (B, C), frame_scores (B, T)."""
        out = []
        for i in range(ensemble_logits.shape[0]):
            out.append(self.process_ensemble_output(
                ensemble_logits=ensemble_logits[i],
                individual_logits=[z[i] for z in individual_logits_list],
                frame_scores=frame_scores[i] if frame_scores.dim() > 1 else frame_scores,
                video_id=video_ids[i] if isinstance(video_ids, list) else f"video_{i}",
                uncertainty=uncertainties[i].item() if uncertainties is not None else 0.0))
        return out

    # ------------------------------------------------------------------ pieces
    def _log(self, event: dict) -> None:
        try:
            if self.telemetry:
                self.telemetry.log_event(event)
        except Exception:
            pass

    def _queue(self, record: dict) -> None:
        try:
            if self.active_learner:
                self.active_learner.queue_for_label(record)
        except Exception:
            pass

    def _determine_alert_level(self, fake_prob: float, confidence: float, uncertainty: float) -> AlertLevel:
        """the alert bands shrink with the uncertainty (factor ``1 - 0.2 * uncertainty``)"""
        factor = 1.0 - 0.2 * uncertainty
        if fake_prob < self.thresholds["safe_max"] * factor:
            return AlertLevel.SAFE
        if fake_prob < self.thresholds["warning_max"] * factor:
            return AlertLevel.WARNING
        if fake_prob < self.thresholds["danger_max"] * factor:
            return AlertLevel.DANGER
        return AlertLevel.CRITICAL

    def _generate_explanation(self, fake_prob: float, confidence: float, uncertainty: float, alert_level: AlertLevel,
                              individual_probs: list) -> str:
        parts = [f"Classification: {ALERT_NAMES[alert_level]}", f"Fake probability: {fake_prob * 100:.1f}%",
                 f"Confidence: {confidence * 100:.1f}%"]
        if uncertainty > 0.5:
            parts.append(f"High uncertainty detected ({uncertainty * 100:.1f}%)")
        if individual_probs:
            parts.append(f"Model agreement: {(1 - np.std(individual_probs)) * 100:.1f}%")
        if confidence < 0.05 and uncertainty > 0.5:
            parts.append("Action: Abstain and request human review or collect more data")
        return " | ".join(parts)
