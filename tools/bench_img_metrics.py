#!/usr/bin/env python
"""Time the image metrics of a test-set pass: 8 frames of 400 x 400 and 8 frames of 260 x 346, MSE + PSNR + SSIM of every frame.

    python tools/bench_img_metrics.py [--reps 20] [--out profiles/img_metrics_bench.json]      on the GPU

In one run and per shape, HIP events around each repetition, 10 warm-up calls of every route first, the median of --reps:
  (a) new        metrics.img_metrics (evd_img_metrics: one call, two kernels, no read-back)
  (b) composed   the same three metrics from PyTorch operations on the device, in float64 after the float32 mapping: the five window
                 means by avg_pool2d on a [B, 15, H, W] stack, S, its mean, the squared differences, amin, log10
  (c) host       where scipy can be imported: the frames copied to the host and tests/img_metric_ref.py (the float64 restatement of the
                 scikit-image algorithm the reference runs there), wall clock, 3 runs
The device-kernel count of (a) and (b) is taken from torch.profiler on one call each (null where the profiler is not available).
Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((8, 400, 400), (8, 260, 346))


def composed(pred, target):
    """compute_img_metric's three metrics without a mask or margin, per image, from torch operations"""
    import torch
    import torch.nn.functional as F
    x = (pred * 2 - 1).clamp(-1, 1).permute(0, 3, 1, 2).double()
    y = (target * 2 - 1).clamp(-1, 1).permute(0, 3, 1, 2).double()
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    rng = torch.where(x.amin(dim=(1, 2, 3)) >= 0, 1.0, 2.0).double()
    psnr = 10 * torch.log10(rng * rng / mse)
    u = F.avg_pool2d(torch.cat([x, y, x * x, y * y, x * y], 1), 7, stride=1)
    ux, uy, uxx, uyy, uxy = u.split(3, 1)
    cn, c1, c2 = 49.0 / 48.0, (0.01 * 2) ** 2, (0.03 * 2) ** 2
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return mse, psnr, s.mean(dim=(1, 2, 3))


def inputs(B, H, W):
    """smooth frames plus noise, float32 [B, H, W, 3]"""
    rs = np.random.RandomState(H)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 0.5 + 0.3 * np.sin(0.05 * xx[None, ..., None] + rs.uniform(0, 6, (B, 1, 1, 3))) * np.cos(0.04 * yy)[None, ..., None]
    pred = (base + 0.05 * rs.standard_normal(base.shape)).astype(np.float32)
    return pred, np.clip(base + 0.05 * rs.standard_normal(base.shape), 0, 1).astype(np.float32)


def kernel_count(fn):
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import metrics as M
    if not torch.cuda.is_available():
        raise SystemExit("bench_img_metrics: needs a GPU")
    try:
        import img_metric_ref as R
    except ImportError:
        R = None
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    fns = {}

    def emit():
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    for B, H, W in SHAPES:
        pred, target = (torch.as_tensor(v, device="cuda") for v in inputs(B, H, W))

        def new(pred=pred, target=target):
            return M.img_metrics(pred, target)

        def comp(pred=pred, target=target):
            return composed(pred, target)

        n, c = new(), comp()
        r = {"max_abs_new_minus_composed": {k: float((n[k] - v).abs().max()) for k, v in zip(("mse", "psnr", "ssim"), c)}}
        r["new_ms"] = timed(new)
        r["composed_ms"] = timed(comp)
        r["new_ms_second_pass"] = timed(new)             # the spread of (a) across the run
        r["speedup_new_over_composed"] = round(r["composed_ms"]["median"] / r["new_ms"]["median"], 2)
        fns[f"{B}x{H}x{W}"] = (new, comp)
        if R is not None:
            def host():
                return R.img_metrics_ref(pred.cpu().numpy(), target.cpu().numpy())
            host()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                h = host()
                ts.append((time.perf_counter() - t0) * 1e3)
            r["host_restatement_ms"] = [round(t, 2) for t in ts]
            r["max_abs_new_minus_host"] = {k: float(np.abs(n[k].cpu().numpy() - h[k]).max()) for k in ("mse", "psnr", "ssim")}
        res["shapes"][f"{B}x{H}x{W}"] = r
    emit()                                               # the times are on disk before the profiler starts
    for key, (new, comp) in fns.items():
        res["shapes"][key]["device_kernels"] = {"new": kernel_count(new), "composed": kernel_count(comp)}
    print(emit())


if __name__ == "__main__":
    main()
