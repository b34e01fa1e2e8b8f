#!/usr/bin/env python3
"""One training epoch of 20 steps at the bench configuration (32 clips x 8 frames x 224 x 224, fp16, uint8 input),
two ways on the same device, interleaved:

  (a) ``EnsembleTrainer.train_epoch``: the metrics accumulate on the device, one host sync at the epoch's end;
  (b) the same ``TrainStep`` loop with the reference's per-step bookkeeping (``src/ensemble_trainer.py:203-211``):
      ``loss.item()`` and three ``.cpu()`` reads after every step, sklearn-free metrics at the end left out.

Also the time of ``EpochMetrics.compute()`` (finalize + the one read-back) at N = 640 and N = 65,536 stored rows.
Prints one JSON line.  Needs a HIP device; timings are host clocks around work that ends in a device synchronise.

    python tools/epoch_sync_ab.py [--steps 20] [--rounds 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
import deepfake_amd  # noqa: E402,F401
from deepfake_amd.losses import WeightedCrossEntropyLoss  # noqa: E402
from deepfake_amd.metrics import EpochMetrics  # noqa: E402
from deepfake_amd.pretrained_detector import PretrainedBackboneDetector  # noqa: E402
from deepfake_amd.trainer import EnsembleTrainer, TrainStep  # noqa: E402
from deepfake_amd.weights import deterministic_init_  # noqa: E402


def make_model(dev):
    torch.manual_seed(0)
    m = PretrainedBackboneDetector("efficientnet_b0", pretrained=False, num_classes=2, dropout_rate=0.5,
                                   compute_dtype="fp16")
    deterministic_init_(m, seed=0)
    return m.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("epoch_sync_ab: needs a HIP device")
    dev = torch.device("cuda", 0)
    x, labels = bench.synthetic_batch(0, dev, "uint8")
    loader = [(x, labels)] * args.steps
    w = torch.tensor([1.0, 1.0])

    with tempfile.TemporaryDirectory() as td:
        trainer = EnsembleTrainer(make_model(dev), device=dev, checkpoint_dir=td)
        opt, _ = trainer.prepare_optimizers(lr=1e-4, weight_decay=1e-5)
        crit = WeightedCrossEntropyLoss(weight=w).to(dev)
        step = TrainStep(make_model(dev), lr=1e-4, weight_decay=1e-5, class_weights=w.to(dev), max_grad_norm=1.0)

        def epoch_a():
            return trainer.train_epoch(loader, opt, crit, 1)

        def epoch_b():
            total, preds, labs, probs = 0.0, [], [], []
            for images, y in loader:
                loss, logits = step(images, y)
                total += loss.item()
                with torch.no_grad():
                    p = F.softmax(logits, dim=1)
                    preds.extend(logits.argmax(dim=1).cpu().numpy())
                    labs.extend(y.cpu().numpy())
                    probs.extend(p[:, 1].cpu().numpy())
            return total / len(loader)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        for _ in range(args.warmup):
            epoch_a()
            epoch_b()
        a, b = [], []
        for _ in range(args.rounds):  # alternating, so drift on a shared host hits both
            a.append(timed(epoch_a))
            b.append(timed(epoch_b))

    fin = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for n in (640, 65536):
        em = EpochMetrics(dev, capacity=n)
        z = torch.randn(n, 2, generator=g, device=dev)
        y = torch.randint(0, 2, (n,), generator=g, device=dev)
        for o in range(0, n, 4096):
            em.update(z[o:o + 4096], y[o:o + 4096])
        em.compute()
        ts = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            em.compute()
            ts.append((time.perf_counter() - t0) * 1e3)
        fin[str(n)] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(t, 4) for t in v]}

    print(json.dumps({"steps": args.steps, "rounds": args.rounds, "config": "32x8x224x224 fp16 uint8",
                      "device_metrics_ms_per_step": summary(a), "per_step_sync_ms_per_step": summary(b),
                      "finalize_ms": fin}))


if __name__ == "__main__":
    main()
