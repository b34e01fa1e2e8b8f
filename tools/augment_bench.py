"""Time ``augment_frames`` on the device against the same chain through Pillow on the host.

    python tools/augment_bench.py [--frames 256] [--size 224] [--iters 50] [--threads 16]

Device: HIP events around ``iters`` back-to-back calls after a warm-up, for (a) every stage on in every row and
(b) crop + flip only; reported per call, with the share of the HBM floor ``2 * N * H * W * 3`` bytes over the
chip's peak rate.  The table upload (two small host-to-device copies) is inside the timed call.  Host: the same
rows through Pillow (resize, flip, ImageEnhance, HSV hue, convert('L'), two resizes) and torch's conv2d for the
blur, on a pool of ``threads`` threads (Pillow releases the GIL in its C loops).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepfake_amd  # noqa: E402,F401
from deepfake_amd import _lib, augment  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def tables(n, size, every_stage, seed=1):
    pi, pf = augment.draw_augment_params(n, (size, size), (size, size), torch.Generator().manual_seed(seed))
    pi[:, 0] = (augment.FLIP | augment.JITTER | augment.GRAY | augment.DOWNUP | augment.BLUR) if every_stage \
        else augment.FLIP
    return pi, pf


def pil_frame(a, pi, pf, size):
    from PIL import Image, ImageEnhance

    i, j, h, w = (int(v) for v in pi[1:5])
    img = Image.fromarray(a).crop((j, i, j + w, i + h)).resize((size, size), Image.BILINEAR)
    if pi[0] & augment.FLIP:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if pi[0] & augment.JITTER:
        for op in pi[5:9]:
            if op == 3:
                hh, s, v = img.convert("HSV").split()
                nh = np.array(hh, dtype=np.uint8) + np.uint8(pi[9])
                img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
            else:
                img = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](img).enhance(float(pf[op]))
    if pi[0] & augment.GRAY:
        g = np.array(img.convert("L"))
        img = Image.fromarray(np.dstack([g, g, g]))
    if pi[0] & augment.DOWNUP:
        img = img.resize((int(pi[11]), int(pi[10])), Image.BILINEAR).resize((size, size), Image.BILINEAR)
    x = np.array(img)
    if pi[0] & augment.BLUR:
        k = torch.from_numpy(pf[3:6])
        k2 = torch.mm(k[:, None], k[None, :]).expand(3, 1, 3, 3)
        t = torch.nn.functional.pad(torch.from_numpy(x).permute(2, 0, 1)[None].float(), (1, 1, 1, 1), mode="reflect")
        x = torch.round(torch.nn.functional.conv2d(t, k2, groups=3))[0].permute(1, 2, 0).to(torch.uint8).numpy()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    n, size = args.frames, args.size
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a HIP device")
    dev = torch.device("cuda:0")
    host = np.random.RandomState(0).randint(0, 256, (n, size, size, 3)).astype(np.uint8)
    src = torch.from_numpy(host).to(dev)
    floor_s = 2.0 * n * size * size * 3 / HBM_PEAK
    res = {"frames": n, "size": size, "iters": args.iters, "hbm_floor_us": floor_s * 1e6,
           "lds_resident": int(_lib.load().dfd_augment_lds_resident(size, size, size, size))}
    for key, every in (("all_stages", True), ("crop_flip", False)):
        pi, pf = tables(n, size, every)
        for _ in range(5):
            augment.augment_frames(src, pi, pf, (size, size))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            augment.augment_frames(src, pi, pf, (size, size))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        res[key] = {"us_per_call": us, "frames_per_s": n / (us * 1e-6), "hbm_floor_share": floor_s * 1e6 / us}
    torch.set_num_threads(1)
    pi, pf = (t.numpy() for t in tables(n, size, True))
    with ThreadPoolExecutor(args.threads) as pool:
        list(pool.map(lambda k: pil_frame(host[k], pi[k], pf[k], size), range(min(n, 32))))
        t0 = time.perf_counter()
        list(pool.map(lambda k: pil_frame(host[k], pi[k], pf[k], size), range(n)))
        dt = time.perf_counter() - t0
    res["pillow_host"] = {"threads": args.threads, "frames_per_s": n / dt}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
