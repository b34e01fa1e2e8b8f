"""Serving on the HIP detector: the pretrained branch of ``app.predict_video`` (``app.py:2027-2223``).

``FrameClassifierService`` is what ``app.load_model(path, 'pretrained')`` + ``predict_video`` do
around the model -- minus face extraction (MTCNN/Haar + video decode are out of scope; the caller
passes the uint8 face crops ``extract_faces_from_video`` returns, or injects that function):

* ``MAX_FRAMES`` (default 8, clamped 1..64) and ``MIN_FACES`` (default 2) gates;
* the crops go to the device as uint8 (1 B/px over PCIe instead of 4) and the app's
  ``/255`` + ImageNet normalisation (``:2084-2085``, ``imagenet_normalize`` ``:1772-1780``) runs
  inside the stem kernel, bit-identical to normalising first (``tests/test_serving.py``);
* ``softmax`` over the 2 logits, fake-class index (``FAKE_CLASS_INDEX`` env > checkpoint
  metadata > 1, ``:1833-1869``), threshold (``calibration_best.json`` next to the checkpoint >
  ``DETECT_FAKE_THRESHOLD`` > 0.5, extreme values ignored unless
  ``ALLOW_EXTREME_CALIBRATION_THRESHOLD``, ``:2096-2109``), borderline / low-confidence abstain
  (``DETECT_ABSTAIN_MARGIN``, ``DETECT_ABSTAIN_CONF``, ``:2173-2210``) and the result dict with
  the same keys, values and descriptions; any exception becomes ``{'error': str(e)}`` (``:2320``).

For an ensemble (a model with ``.models``) the app does not stop there: unless
``DISABLE_ENHANCED_AGENT`` is set, ``EnhancedDecisionAgent`` (``agent.py``) replaces ``pred_class``,
``confidence`` and ``description`` and fills ``enhanced_agent`` (``:2118-2171``).  ``decide(...,
agent_inputs=, agent=, video_id=)`` restates that step.  The app gets the members' logits by running
every member a second time after ``MODEL(x)``; a model with ``forward_members``
(``pretrained_detector.EnsembleDetector``) runs each member once instead, and ``ensemble_decide``
turns their outputs into the ensemble's logits and scores and a decision block per video in one
launch (``dfd::ensemble_decide``, ``csrc/k_ensemble.hip``): one ``.cpu()`` of that block serves a whole
group of videos.  The kernel holds the fp32 values only; what the reference computes in Python
floats (``np.std``, agreement, adjusted probability, thresholds, formatted strings) stays on the host
in double.  A model that only has ``.models`` (a stub) takes the app's literal route: the forward,
then each member once more.  ``ensemble_decide_host`` is the same contract in the torch CPU ops the
reference uses -- the path for CPU tensors and the yardstick of the kernel.

``predict_batch`` is the batched multi-video variant: videos with the same face
count go through ONE forward of shape (videos, T, 3, H, W); in eval mode the clips do not
interact, so each result equals the single-video one.
"""
from __future__ import annotations

import json
import os
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------ env helpers (app.py:352, 1802-1906)
def _safe_int(x):
    try:
        return int(x)
    except Exception:
        return None


def _env_float(name):
    v = os.environ.get(name)
    if v is None:
        return None
    v = str(v).strip()
    if not v:
        return None
    try:
        return float(v)
    except Exception:
        return None


def _env_int(name):
    v = os.environ.get(name)
    if v is None:
        return None
    v = str(v).strip()
    if not v:
        return None
    return _safe_int(v)


def _env_flag(name):
    return str(os.environ.get(name, "")).strip().lower() in ("1", "true", "yes", "y")


def fake_class_index(num_classes=2, load_stats=None):
    nc = max(1, int(num_classes))
    idx = _env_int("FAKE_CLASS_INDEX")
    if idx is not None and 0 <= idx < nc:
        return int(idx)
    det = (load_stats or {}).get("fake_class_index_detected")
    if det is not None:
        d = _safe_int(det)
        if d is not None and 0 <= d < nc:
            return d
    return 1 if nc > 1 else 0


def threshold_fallback(default=0.5):
    t = _env_float("DETECT_FAKE_THRESHOLD")
    if t is not None and 0.0 <= float(t) <= 1.0:
        return float(t)
    return float(default)


def calibration_threshold(checkpoint_path):
    """``best_thr_accuracy`` of calibration_best.json next to the checkpoint (app.py:1783-1799)."""
    if not checkpoint_path:
        return None
    try:
        cand = Path(checkpoint_path).parent / "calibration_best.json"
        if cand.exists():
            thr = json.loads(cand.read_text(encoding="utf-8")).get("best_thr_accuracy")
            if thr is not None:
                t = float(thr)
                return t if 0.0 <= t <= 1.0 else None
    except Exception:
        return None
    return None


def max_frames_setting():
    try:
        m = int(os.environ.get("MAX_FRAMES", "8"))
    except Exception:
        m = 8
    return max(1, min(64, int(m)))


def imagenet_normalize(frames: torch.Tensor) -> torch.Tensor:
    """``app.imagenet_normalize`` (float frames in [0,1], (T,C,H,W) or (B,T,C,H,W))."""
    mean = torch.tensor(IMAGENET_MEAN, device=frames.device, dtype=frames.dtype)
    std = torch.tensor(IMAGENET_STD, device=frames.device, dtype=frames.dtype)
    if frames.dim() == 4:
        return (frames - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    if frames.dim() == 5:
        return (frames - mean.view(1, 1, 3, 1, 1)) / std.view(1, 1, 3, 1, 1)
    raise ValueError(f"Unsupported frames shape for normalization: {tuple(frames.shape)}")


ENSEMBLE_BLOCK_BASE = 5  # decision-block words in front of the per-member probabilities (include/dfd_hip.h)


def ensemble_decide_host(member_logits, member_scores, weights, method, fake_idx, temperature):
    """``dfd::ensemble_decide`` in the torch ops of the reference, on the tensors' own device (CPU in the tests):
    member logits (M, V, 2), member scores (M, V, T), raw weights (M) or None -> (logits (V, 2), scores (V, T),
    block (V, 5 + 2M)).  Combination: ``EnsembleDetector.forward`` (src/pretrained_detector.py:196-216); block:
    [0] / [1] the app's prob_fake / prob_real (app.py:2090-2094), [2] the agent's fake_prob at ``logits /
    temperature``, [3] the members' modal argmax, [4] M, [5 + m] the app's ind_probs (:2143), [5 + M + m] the agent's
    individual_probs."""
    zl = member_logits.detach().float()
    zs = member_scores.detach().float()
    if zl.dim() != 3 or zs.dim() != 3 or zl.shape[:2] != zs.shape[:2]:
        raise ValueError(f"needs (M, V, C) logits and (M, V, T) scores, got {tuple(zl.shape)} and {tuple(zs.shape)}")
    M, V, C = zl.shape
    if not 1 <= M <= 8 or C != 2 or not 1 <= zs.shape[2] <= 64 or V < 1:
        raise ValueError("needs 1 <= M <= 8 members, C == 2 classes, 1 <= T <= 64 frames and V >= 1 videos")
    if int(fake_idx) not in (0, 1) or not float(temperature) > 0.0:
        raise ValueError("needs fake_idx 0 or 1 and temperature > 0")
    fake_idx, temperature = int(fake_idx), float(temperature)
    mode = torch.mode(zl.argmax(dim=-1), dim=0)[0]
    if method == "average":
        logits, scores = zl.mean(dim=0), zs.mean(dim=0)
    elif method == "weighted":
        if weights is None:
            raise ValueError("the weighted method needs the ensemble's weight vector")
        w = F.softmax(weights.detach().float(), dim=0)
        logits, scores = (zl * w.view(-1, 1, 1)).sum(dim=0), (zs * w.view(-1, 1, 1)).sum(dim=0)
    elif method == "voting":
        logits, scores = F.one_hot(mode, num_classes=2).float(), zs.mean(dim=0)
    else:
        raise ValueError(f"Unknown ensemble method: {method}")
    probs = torch.softmax(logits, dim=1)
    block = torch.empty(V, ENSEMBLE_BLOCK_BASE + 2 * M, dtype=torch.float32, device=zl.device)
    block[:, 0] = probs[:, fake_idx]
    block[:, 1] = probs[:, 1 - fake_idx]
    block[:, 2] = F.softmax(logits / temperature, dim=1)[:, fake_idx]
    block[:, 3] = mode.float()
    block[:, 4] = float(M)
    block[:, 5:5 + M] = torch.softmax(zl, dim=2)[:, :, fake_idx].T
    block[:, 5 + M:] = F.softmax(zl / temperature, dim=2)[:, :, fake_idx].T
    return logits, scores, block


def ensemble_decide(member_logits, member_scores, weights, method, fake_idx=1, temperature=1.0):
    """The HIP kernel for device tensors, ``ensemble_decide_host`` for CPU tensors (stub members in tests)."""
    if member_logits.is_cuda:
        from . import ops  # noqa: F401  (registers torch.ops.dfd.*)

        return torch.ops.dfd.ensemble_decide(member_logits, member_scores, weights, method, int(fake_idx),
                                             float(temperature))
    return ensemble_decide_host(member_logits, member_scores, weights, method, fake_idx, temperature)


def block_agent_inputs(row):
    """One video's decision-block row (host floats) -> the ``agent_inputs`` of ``decide``."""
    row = [float(v) for v in row]
    M = (len(row) - ENSEMBLE_BLOCK_BASE) // 2
    if len(row) != ENSEMBLE_BLOCK_BASE + 2 * M or M < 1 or row[4] != float(M):
        raise ValueError(f"not a decision block row: {len(row)} words, spare word {row[4] if len(row) > 4 else None}")
    return {"prob_fake": row[0], "prob_real": row[1], "fake_prob": row[2], "ind_probs": row[5:5 + M],
            "individual_probs": row[5 + M:5 + 2 * M]}


_DEFAULT_AGENT = None


def default_agent():
    """The app's module-level ``ENHANCED_AGENT = EnhancedDecisionAgent()`` (app.py:115)."""
    global _DEFAULT_AGENT
    if _DEFAULT_AGENT is None:
        from .agent import EnhancedDecisionAgent

        _DEFAULT_AGENT = EnhancedDecisionAgent()
    return _DEFAULT_AGENT


def _agent_step(agent, agent_inputs, logits_row, thr, fake_idx, video_id):
    """app.py:2122-2171 minus the try/except around it: the payload dict.  ``agent_inputs`` (a dict, or a callable
    returning one -- called here, so that a member failing on its second run is caught like in the app):
    either the logits of the literal route, ``{'individual_logits': [(C) or (1, C) ...], 'frame_scores': ...}``, or
    the fp32 values of a decision block (``block_agent_inputs``)."""
    old = getattr(agent, "decision_threshold", 0.5)
    try:
        try:
            agent.decision_threshold = float(thr)
        except Exception:
            pass
        inputs = agent_inputs() if callable(agent_inputs) else agent_inputs
        try:
            setattr(agent, "fake_class_index", int(fake_idx))
        except Exception:
            pass
        if "individual_logits" in inputs:
            ind_logits = [z.detach().float().cpu().reshape(-1) for z in inputs["individual_logits"]]
            ind_probs = [float(torch.softmax(z, dim=0)[int(fake_idx)].item()) for z in ind_logits]
        else:
            ind_logits = None
            ind_probs = [float(p) for p in inputs["ind_probs"]]
        uncertainty = float(np.std(ind_probs)) if len(ind_probs) >= 2 else 0.0
        scores = inputs.get("frame_scores")
        if scores is not None and hasattr(scores, "dim") and scores.dim() > 1:
            scores = scores.squeeze(0)
        if ind_logits is not None:
            pred = agent.process_ensemble_output(
                ensemble_logits=logits_row.detach().float().cpu().reshape(1, -1), individual_logits=ind_logits,
                frame_scores=scores, video_id=str(video_id), uncertainty=uncertainty)
        else:
            pred = agent.process_probs(float(inputs["fake_prob"]), [float(p) for p in inputs["individual_probs"]],
                                       frame_scores=scores, video_id=str(video_id), uncertainty=uncertainty)
        return {"is_fake": bool(pred.is_fake), "ensemble_prob": float(pred.ensemble_prob),
                "confidence": float(pred.confidence),
                "alert_level": getattr(pred.alert_level, "name", str(pred.alert_level)),
                "uncertainty": float(pred.uncertainty), "explanation": str(pred.explanation)}
    finally:
        try:
            agent.decision_threshold = old
        except Exception:
            pass


def decide(logits_row: torch.Tensor, num_faces: int, checkpoint_path=None, load_stats=None, ensemble=False,
           agent_inputs=None, agent=None, video_id=None):
    """Post-processing of ONE video's logits (app.py:2090-2223): probabilities, threshold, abstain
    rules, result dict.  ``agent_inputs`` (``_agent_step``) adds the enhanced agent's step of the ensemble
    branch (``:2118-2171``) with ``agent`` (default: one module-level ``EnhancedDecisionAgent()``, as the app's)
    and ``video_id``; where it carries ``prob_fake`` / ``prob_real`` (a decision block), ``logits_row`` may be None."""
    try:
        abstain_conf = float(os.environ.get("DETECT_ABSTAIN_CONF", "0.60"))
    except Exception:
        abstain_conf = 0.60
    try:
        abstain_margin = float(os.environ.get("DETECT_ABSTAIN_MARGIN", "0.0"))
    except Exception:
        abstain_margin = 0.0
    abstain_margin = max(0.0, min(0.5, float(abstain_margin)))

    if isinstance(agent_inputs, dict) and "prob_fake" in agent_inputs:  # the decision block's fp32 values
        fake_idx = fake_class_index(2, load_stats)
        prob_fake, prob_real = float(agent_inputs["prob_fake"]), float(agent_inputs["prob_real"])
    else:
        probs = torch.softmax(logits_row.detach().float().cpu().reshape(1, -1), dim=1)
        nc = int(probs.shape[1])
        fake_idx = fake_class_index(nc, load_stats)
        real_idx = (1 - int(fake_idx)) if nc == 2 else 0
        prob_fake = float(probs[0, int(fake_idx)].item())
        prob_real = float(probs[0, int(real_idx)].item())
    thr = calibration_threshold(checkpoint_path)
    thr = threshold_fallback(0.5) if thr is None else float(thr)
    thr = float(threshold_fallback(thr))
    if not _env_flag("ALLOW_EXTREME_CALIBRATION_THRESHOLD") and (float(thr) < 0.05 or float(thr) > 0.95):
        thr = 0.5
    is_fake = bool(prob_fake >= float(thr))
    pred_class = 1 if is_fake else 0
    confidence = float(prob_fake if is_fake else prob_real)
    description = (f"Pretrained detector (thr={thr:.2f})" if not ensemble
                   else f"Ensemble pretrained detector (thr={thr:.2f})")
    agent_payload = None
    if agent_inputs is not None and not _env_flag("DISABLE_ENHANCED_AGENT"):
        try:
            agent_payload = _agent_step(agent if agent is not None else default_agent(), agent_inputs, logits_row,
                                        thr, fake_idx, "" if video_id is None else video_id)
            description = agent_payload.get("explanation") or description
            pred_class = int(agent_payload.get("is_fake"))
            confidence = float(agent_payload.get("confidence", confidence))
        except Exception:
            agent_payload = None
    if abstain_margin > 0.0 and abs(float(prob_fake) - float(thr)) <= float(abstain_margin):
        return {"prediction": "Uncertain", "verdict_yes_no": "Unsure",
                "description": (f"Borderline score (prob_fake={prob_fake * 100:.1f}%, thr={thr:.2f} ± "
                                f"{abstain_margin:.2f}). Manual review recommended.\n\n" + (description or "")),
                "pred_class": None, "confidence": float(confidence), "prob_real": float(prob_real),
                "prob_fake": float(prob_fake), "num_faces": int(num_faces), "threshold": float(thr),
                "enhanced_agent": agent_payload, "abstained": True}
    if confidence < float(abstain_conf):
        return {"prediction": "Uncertain", "verdict_yes_no": "Unsure",
                "description": (f"Low confidence ({confidence * 100:.1f}%). This video may be out-of-domain "
                                "(different compression, face quality, lighting, or manipulation type). Manual "
                                "review recommended.\n\n" + (description or "")),
                "pred_class": None, "confidence": float(confidence), "prob_real": float(prob_real),
                "prob_fake": float(prob_fake), "num_faces": int(num_faces), "threshold": float(thr),
                "enhanced_agent": agent_payload, "abstained": True}
    return {"prediction": "Deepfake" if pred_class == 1 else "Real",
            "verdict_yes_no": "Yes" if pred_class == 1 else "No", "description": description,
            "pred_class": int(pred_class), "confidence": float(confidence), "prob_real": float(prob_real),
            "prob_fake": float(prob_fake), "num_faces": int(num_faces), "threshold": float(thr),
            "enhanced_agent": agent_payload}


def _too_few(num_faces):
    try:
        min_faces = int(os.environ.get("MIN_FACES", "2"))
    except Exception:
        min_faces = 2
    min_faces = max(1, int(min_faces))
    if num_faces < min_faces:
        return {"prediction": "Uncertain", "verdict_yes_no": "Unsure",
                "description": (f"Not enough faces/frames detected for a stable decision (num_faces={num_faces}, "
                                f"min_faces={min_faces}). Try a clearer face shot, better lighting, or a longer clip."),
                "pred_class": None, "confidence": None, "prob_real": None, "prob_fake": None,
                "num_faces": int(num_faces), "abstained": True}
    return None


class FrameClassifierService:
    """Model + checkpoint context of the app's pretrained serving path on one device."""

    def __init__(self, model, checkpoint_path=None, load_stats=None, device=None, agent=None):
        self.model = model.eval()
        self.checkpoint_path = checkpoint_path
        self.load_stats = load_stats or {}
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        self.agent = agent  # None: the module-level default, as the app's ENHANCED_AGENT

    @classmethod
    def from_checkpoint(cls, path, device="cuda", compute_dtype="fp32", meta=None):
        """An ensemble checkpoint (``models.<i>.`` keys after prefix normalisation) loads through
        ``checkpoint.load_ensemble``, anything else through ``load_pretrained``."""
        from . import checkpoint as ck

        obj = ck.read_checkpoint(path)
        if ck.is_ensemble_state_dict(ck.normalize_state_dict_keys(ck.extract_state_dict(obj))):
            model, stats = ck.load_ensemble(obj, device=device, compute_dtype=compute_dtype, meta=meta)
        else:
            model, stats = ck.load_pretrained(obj, device=device, compute_dtype=compute_dtype,
                                              checkpoint_name=str(path), meta=meta)
        return cls(model, checkpoint_path=str(path), load_stats={**stats, "checkpoint": str(path)}, device=device)

    # -- tensor handover (app.py:2084-2086)
    def _frames(self, faces_list):
        """(V, T, H, W, 3) uint8 crops -> the model's input (V, T, 3, H, W) on the device."""
        u8 = torch.from_numpy(np.ascontiguousarray(np.stack(faces_list))).to(self.device, non_blocking=True)
        x = u8.permute(0, 1, 4, 2, 3)  # channels-last strides, as the app's permute
        if getattr(self.model, "accepts_uint8_frames", False):
            return x  # normalised inside the stem kernel
        return imagenet_normalize(x.float() / 255.0)  # a model without the fused input path

    @torch.no_grad()
    def _logits(self, faces_list):
        out = self.model(self._frames(faces_list))
        logits = out[0] if isinstance(out, tuple) else out
        return logits.float().cpu()

    # -- the group of videos behind one forward
    def _decide_group(self, faces_list, video_ids):
        """One forward for videos of equal shape -> their result dicts.  Plain model: ``decide`` on each logits row.
        Ensemble: with the agent's inputs -- from the decision block of ``forward_members`` (each member once, one
        launch, ONE read-back for the group) or, for a model that only has ``.models``, by the app's literal route
        (the forward, then every member once more; a failure there costs the agent's payload, not the result)."""
        ensemble = hasattr(self.model, "models")
        kw = dict(checkpoint_path=self.checkpoint_path, load_stats=self.load_stats, ensemble=ensemble)
        nums = [int(len(f)) for f in faces_list]
        if not ensemble:
            logits = self._logits(faces_list)
            return [decide(logits[j], nums[j], **kw) for j in range(len(faces_list))]
        x = self._frames(faces_list)
        if hasattr(self.model, "forward_members"):
            agent = self.agent if self.agent is not None else default_agent()
            with torch.no_grad():
                out = self.model.forward_members(x, fake_idx=fake_class_index(2, self.load_stats),
                                                 temperature=float(getattr(agent, "temperature", 1.0)),
                                                 return_block=True)
            rows = out[4].float().cpu().tolist()  # the group's single device read
            return [decide(None, nums[j], agent_inputs=block_agent_inputs(rows[j]), agent=self.agent,
                           video_id=video_ids[j], **kw) for j in range(len(faces_list))]
        with torch.no_grad():
            out = self.model(x)
        logits, scores = (out[0], out[1]) if isinstance(out, tuple) else (out, None)
        logits = logits.float().cpu()
        again = {}

        def members():  # runs inside decide's agent step, once per group
            if "error" in again:
                raise again["error"]
            if "logits" not in again:
                try:
                    with torch.no_grad():
                        again["logits"] = [m(x)[0].float().cpu() for m in self.model.models]
                except Exception as e:
                    again["error"] = e
                    raise
            return again["logits"]

        results = []
        for j in range(len(faces_list)):
            def inputs(j=j):
                return {"individual_logits": [z[j] for z in members()],
                        "frame_scores": None if scores is None else scores[j].float().cpu()}

            results.append(decide(logits[j], nums[j], agent_inputs=inputs, agent=self.agent, video_id=video_ids[j],
                                  **kw))
        return results

    def predict_faces(self, faces: np.ndarray, video_id: str = "") -> dict:
        try:
            num_faces = int(len(faces))
            if num_faces == 0:
                return {"error": "No faces detected in video"}
            few = _too_few(num_faces)
            if few is not None:
                return few
            return self._decide_group([faces], [video_id])[0]
        except Exception as e:
            return {"error": str(e)}

    def predict_video(self, video_path, extract_faces) -> dict:
        """``predict_video`` with the face extractor injected (``extract_faces(path, max_frames=)``)."""
        try:
            faces = extract_faces(video_path, max_frames=max_frames_setting())
        except Exception as e:
            return {"error": str(e)}
        return self.predict_faces(faces, video_id=str(Path(video_path).name))

    def predict_batch(self, faces_per_video, video_ids=None) -> list:
        """Batched multi-video serving: one forward per group of videos with equal face count."""
        results = [None] * len(faces_per_video)
        ids = [""] * len(faces_per_video) if video_ids is None else [str(v) for v in video_ids]
        groups = {}
        for i, faces in enumerate(faces_per_video):
            n = int(len(faces))
            if n == 0:
                results[i] = {"error": "No faces detected in video"}
                continue
            few = _too_few(n)
            if few is not None:
                results[i] = few
                continue
            groups.setdefault((n,) + tuple(np.shape(faces)[1:]), []).append(i)
        for _, idxs in groups.items():
            try:
                group = self._decide_group([faces_per_video[i] for i in idxs], [ids[i] for i in idxs])
                for j, i in enumerate(idxs):
                    results[i] = group[j]
            except Exception as e:
                for i in idxs:
                    results[i] = {"error": str(e)}
        return results
