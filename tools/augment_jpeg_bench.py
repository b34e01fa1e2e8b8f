"""Time the augmentation launch with and without the JPEG recompression stage.

    python tools/augment_jpeg_bench.py [--frames 256] [--size 224] [--iters 30] [--quality 75] [--other-lib PATH]

Tables from ``draw_augment_params`` (the reference's probabilities), one launch per measurement between HIP events,
the runs interleaved round by round after a warm-up, the median over ``iters`` rounds reported:
``augment_frames`` (this build), ``augment_frames_jpeg`` with every frame at ``quality``, the same with the drawn
qualities of ``draw_jpeg_quality`` (half the frames skip the stage), and, with ``--other-lib``, ``dfd_augment_frames``
of a ``libdfd_hip.so`` built from another commit, to compare the kernel without the stage across builds.  Every
run goes through the C ABI on preallocated buffers, so nothing but the two or three table copies and the launch is
timed.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepfake_amd  # noqa: E402,F401
from deepfake_amd import _lib, augment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--other-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_jpeg_bench needs a HIP device")
    n, size = args.frames, args.size
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g).to(dev)
    pi, pf = augment.draw_augment_params(n, (size, size), (size, size), g)
    drawn = augment.draw_jpeg_quality(n, g)
    fixed = torch.full((n,), args.quality, dtype=torch.int32)
    out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=dev)
    nbytes = int(lib.dfd_augment_jpeg_scratch_bytes(n, size, size, size, size))
    assert nbytes >= int(lib.dfd_augment_scratch_bytes(n, size, size, size, size)) > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = _lib.stream_of(dev)
    head = (stream, src.data_ptr(), n, size, size, pi.data_ptr(), pf.data_ptr())
    tail = (size, size, out.data_ptr(), scratch.data_ptr(), nbytes)

    runs = {"augment_frames": lambda: lib.dfd_augment_frames(*head, *tail),
            f"augment_frames_jpeg_q{args.quality}": lambda: lib.dfd_augment_frames_jpeg(*head, fixed.data_ptr(), *tail),
            "augment_frames_jpeg_drawn": lambda: lib.dfd_augment_frames_jpeg(*head, drawn.data_ptr(), *tail)}
    if args.other_lib:
        other = ctypes.CDLL(os.path.abspath(args.other_lib))
        other.dfd_augment_frames.restype = ctypes.c_int
        other.dfd_augment_frames.argtypes = _lib._SIGS["dfd_augment_frames"][1]
        runs = {"other_lib_augment_frames": lambda: other.dfd_augment_frames(*head, *tail), **runs}
    times = {k: [] for k in runs}
    for it in range(args.iters + 5):
        for key, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise SystemExit(f"{key}: {lib.dfd_last_error().decode(errors='replace')}")
            if it >= 5:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    res = {"frames": n, "size": size, "iters": args.iters, "jpeg_frames_drawn": int((drawn != 0).sum())}
    for key, t in times.items():
        res[key] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
