#!/usr/bin/env python
"""Time one LPIPS call per backbone at the size of a test-set frame: B = 1, 400 x 400, synthetic backbone weights.

    python tools/bench_lpips_vgg.py [--reps 30] [--out profiles/lpips_vgg_bench.json]      on the GPU

Per route 10 warm-up calls, then --reps calls, each between two HIP events; the median, minimum and maximum in milliseconds:
  vgg, alex                    metrics.LPIPS(net=...), the spatial average (evd_lpips)
  vgg_spatial, alex_spatial    the same models with spatial=True (evd_lpips_spatial, per-layer maps not requested)
The convolutions' work is derived from the layer tables (2 M K N per convolution, both frames).  `call_tflops` is that work over the WHOLE
call's time -- pools, distance kernels and launch gaps included -- and `call_fraction_of_f32_matrix_peak` states it against the
157.3 TFLOP/s float32 matrix peak: a lower bound on what the convolution kernel itself reaches.  Prints one JSON line; --out also writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 1, 400, 400
PEAK_F32_MATRIX_TFLOPS = 157.3
# Cin, Cout, kernel, stride, pad, (pool window, stride) in front
ALEX = ((3, 64, 11, 4, 2, None), (64, 192, 5, 1, 2, (3, 2)), (192, 384, 3, 1, 1, (3, 2)), (384, 256, 3, 1, 1, None), (256, 256, 3, 1, 1, None))
VGG = tuple((ci, co, 3, 1, 1, (2, 2) if l in (2, 4, 7, 10) else None) for l, (ci, co) in enumerate(
    ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512), (512, 512),
     (512, 512))))


def conv_flop(layers, B, H, W):
    """2 M K N summed over the convolutions, for the 2 B frames of a call"""
    h, w, total = H, W, 0
    for ci, co, k, s, p, pool in layers:
        if pool:
            h, w = (h - pool[0]) // pool[1] + 1, (w - pool[0]) // pool[1] + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += 2 * (2 * B * h * w) * (k * k * ci) * co
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import metrics as M
    from evdeblurnerf_amd import weights as Wt
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_vgg: needs a GPU")
    rs = np.random.RandomState(4300)
    pred = torch.as_tensor(rs.uniform(0, 1, (B, H, W, 3)).astype(np.float32), device="cuda")
    target = torch.as_tensor(np.clip(pred.cpu().numpy() + 0.1 * rs.standard_normal((B, H, W, 3)), 0, 1).astype(np.float32), device="cuda")
    res = {"shape": [B, H, W], "reps": a.reps, "device": torch.cuda.get_device_name(0), "peak_f32_matrix_tflops": PEAK_F32_MATRIX_TFLOPS, "routes": {}}

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

    for net, layers, sd, chns in (("vgg", VGG, Wt.make_lpips_vgg16_state_dict(4300), (64, 128, 256, 512, 512)),
                                  ("alex", ALEX, Wt.make_lpips_alexnet_state_dict(3800), (64, 192, 384, 256, 256))):
        heads = {f"lin{l}.model.1.weight": rs.uniform(0, 0.1, size=(1, c, 1, 1)).astype(np.float32) for l, c in enumerate(chns)}
        flop = conv_flop(layers, B, H, W)
        for tag, spatial in ((net, False), (net + "_spatial", True)):
            model = M.LPIPS(sd, heads, net=net, spatial=spatial)
            r = {"ms": timed(lambda: model(pred, target)), "conv_gflop_per_call": round(flop / 1e9, 2)}
            r["call_tflops"] = round(flop / (r["ms"]["median"] * 1e-3) / 1e12, 2)
            r["call_fraction_of_f32_matrix_peak"] = round(r["call_tflops"] / PEAK_F32_MATRIX_TFLOPS, 3)
            res["routes"][tag] = r
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
