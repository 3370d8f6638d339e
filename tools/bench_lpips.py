#!/usr/bin/env python
"""Time LPIPS of a test-set pass: 8 frame pairs of 400 x 400 (AlexNet backbone, version 0.1), synthetic backbone weights.

    python tools/bench_lpips.py [--reps 20] [--out profiles/lpips_bench.json]      on the GPU

In one run, HIP events around each repetition, 10 warm-up calls of every route first, the median of --reps:
  (a) new        metrics.LPIPS (evd_lpips: five implicit-GEMM convolutions on the float32 MFMA, two pools, five distance kernels, one
                 finish launch; no read-back)
  (b) composed   the same network from PyTorch operations on the device (conv2d, max_pool2d, the normalised distance), float32
  (c) host       the reference's route: the frames copied to the host and the restated network (tests/lpips_ref.py) in float32 on the
                 CPU, wall clock, 3 runs
The convolutions' work is derived from the layer shapes (2 M K N per layer, both frames); the achieved rate of (a) -- the whole call, the
pools and the distance included -- is stated against the 157.3 TFLOP/s float32 matrix peak.  Prints one JSON line; --out also writes it."""
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

SHAPES = ((8, 400, 400),)
PEAK_F32_MATRIX_TFLOPS = 157.3
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))


def conv_flop(B, H, W):
    """2 M K N summed over the five layers, for the 2 B frames of a call"""
    h, w, total = H, W, 0
    for ci, co, k, s, p, pool in LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += 2 * (2 * B * h * w) * (k * k * ci) * co
    return total


def composed(pred, target, sd, lins, shift, scale):
    import torch
    import torch.nn.functional as F

    def feats(im):
        h = ((im * 2 - 1).clamp(-1, 1).permute(0, 3, 1, 2) - shift) / scale
        outs = []
        for (ci, co, k, s, p, pool), idx in zip(LAYERS, (0, 3, 6, 8, 10)):
            if pool:
                h = F.max_pool2d(h, 3, 2)
            h = torch.relu(F.conv2d(h, sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"], stride=s, padding=p))
            outs.append(h)
        return outs

    val = 0
    for a, b, lin in zip(feats(pred), feats(target), lins):
        na = torch.sqrt((a ** 2).sum(dim=1, keepdim=True))
        nb = torch.sqrt((b ** 2).sum(dim=1, keepdim=True))
        val = val + (((a / (na + 1e-10) - b / (nb + 1e-10)) ** 2) * lin).sum(dim=1).mean(dim=(1, 2))
    return val


def inputs(B, H, W):
    """smooth frames plus noise, float32 [B, H, W, 3]"""
    rs = np.random.RandomState(H)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 0.5 + 0.3 * np.sin(0.05 * xx[None, ..., None] + rs.uniform(0, 6, (B, 1, 1, 3))) * np.cos(0.04 * yy)[None, ..., None]
    pred = (base + 0.05 * rs.standard_normal(base.shape)).astype(np.float32)
    return pred, np.clip(base + 0.05 * rs.standard_normal(base.shape), 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import metrics as M
    from evdeblurnerf_amd import weights as Wt
    import lpips_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: needs a GPU")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    backbone = Wt.make_lpips_alexnet_state_dict(3800)
    rs = np.random.RandomState(3801)
    lins = [rs.uniform(0, 0.1, size=(c,)).astype(np.float32) for c in (64, 192, 384, 256, 256)]      # non-negative, like the trained heads
    model = M.LPIPS(backbone, {f"lin{l}.model.1.weight": v.reshape(1, -1, 1, 1) for l, v in enumerate(lins)})
    sd = {k: torch.as_tensor(v, device="cuda") for k, v in backbone.items()}
    dlins = [torch.as_tensor(v, device="cuda").reshape(1, -1, 1, 1) for v in lins]
    shift = torch.tensor(M.LPIPS.SHIFT, device="cuda").reshape(1, 3, 1, 1)
    scale = torch.tensor(M.LPIPS.SCALE, device="cuda").reshape(1, 3, 1, 1)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "peak_f32_matrix_tflops": PEAK_F32_MATRIX_TFLOPS, "shapes": {}}

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
            return model(pred, target)

        def comp(pred=pred, target=target):
            return composed(pred, target, sd, dlins, shift, scale)

        n, c = new(), comp()
        torch.cuda.synchronize()
        flop = conv_flop(B, H, W)
        r = {"conv_gflop_per_call": round(flop / 1e9, 2), "conv_gflop_per_pair": round(flop / 1e9 / B, 2),
             "max_rel_new_minus_composed": float(((n - c.double()).abs() / n).max())}
        r["new_ms"] = timed(new)
        r["composed_ms"] = timed(comp)
        r["new_ms_second_pass"] = timed(new)             # the spread of (a) across the run
        r["speedup_new_over_composed"] = round(r["composed_ms"]["median"] / r["new_ms"]["median"], 2)
        r["new_tflops"] = round(flop / (r["new_ms"]["median"] * 1e-3) / 1e12, 2)
        r["new_fraction_of_f32_matrix_peak"] = round(r["new_tflops"] / PEAK_F32_MATRIX_TFLOPS, 3)
        r["composed_tflops"] = round(flop / (r["composed_ms"]["median"] * 1e-3) / 1e12, 2)

        def host():
            return R.lpips(pred.cpu().numpy(), target.cpu().numpy(), backbone, lins, M.LPIPS.SHIFT, M.LPIPS.SCALE, dtype=torch.float32)
        hv, _ = host()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            host()
            ts.append((time.perf_counter() - t0) * 1e3)
        r["host_restatement_f32_ms"] = [round(t, 2) for t in ts]
        r["host_threads"] = torch.get_num_threads()
        r["max_rel_new_minus_host"] = float(np.abs(n.cpu().numpy() - hv).max() / np.abs(hv).max())
        res["shapes"][f"{B}x{H}x{W}"] = r
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
