#!/usr/bin/env python
"""Time the 8-bit pictures of a test-set / video pass: depth pictures (inverted, one maximum, colour map) + error maps (maximum per frame,
colour map) + the video's normalised RGB frames, for 8 frames of 400 x 400 and, if memory allows, 120.

    python tools/bench_frames.py [--reps 20] [--out profiles/frames_bench.json]      on the GPU
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_frames.py --frames 120 --reps 5 --no-profiler --no-host
                                                                                      (profiles/frames_kernel_stats.csv: per-kernel times)

In one run and per shape, HIP events around each repetition, 10 warm-up calls of every route first, routes (a) and (b) alternating inside
the timed loop, the median, quartiles, minimum and maximum of --reps:
  (a) new        frames.depth_images + frames.error_maps + frames.video_frames (evd_frame_range / evd_frame_map: two launches and a finish
                 per picture kind, no full-size temporary)
  (b) composed   the same statements from PyTorch operations on the device
  (c) host       the reference's statements through the host: .cpu().numpy() of the float32 frames, then tests/frames_ref.py (NumPy),
                 wall clock around work that ends synchronised, copy included, 3 runs
`bytes` is what (a) must move, computed from the shape (two reads of every source, one write of every picture); new_gbps is bytes over
the median of (a): a whole-call rate with launch gaps and allocations inside, not a kernel's share of peak.  The device-kernel count of
(a) and (b) comes from torch.profiler on one call each (null where the profiler is not available).  The pictures of (a) are compared with
(c) byte for byte, those of (b) too (PyTorch's reduction order is its own: the count is reported, not asserted).
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

H, W = 400, 400


def composed(rgbs, gts, disps, lut):
    """the reference's statements as PyTorch device operations"""
    import torch

    def to8b(x):
        return (255 * x.clamp(0, 1)).to(torch.uint8)

    d = 1. - disps
    depth = lut[(255 - to8b(d / d.max())).long()]
    e = ((rgbs - gts) ** 2).mean(-1)
    err = lut[(255 - to8b(e / e.amax(dim=(1, 2), keepdim=True))).long()]
    mn = rgbs.min()
    video = to8b((rgbs - mn) / (rgbs.max() - mn))
    return depth, err, video


def host(rgbs, gts, disps, lut, R):
    """the reference's route: float32 frames to the host, NumPy there"""
    r, g, d = rgbs.cpu().numpy(), gts.cpu().numpy(), disps.cpu().numpy()
    return R.depth_images(d, True, "all", lut), R.error_maps(r, g, lut), R.video_frames(r)


def inputs(N, H, W, dev):
    """smooth frames plus noise generated on the device from a seed: rgbs, gts [N, H, W, 3], disps [N, H, W]"""
    import torch
    gen = torch.Generator(device=dev).manual_seed(1000 + N)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ph = torch.rand((N, 1, 1, 3), generator=gen, device=dev) * 6
    base = 0.5 + 0.3 * torch.sin(0.05 * xx[None, ..., None] + ph) * torch.cos(0.04 * yy)[None, ..., None]
    rgbs = base + 0.05 * torch.randn(base.shape, generator=gen, device=dev)
    gts = (base + 0.05 * torch.randn(base.shape, generator=gen, device=dev)).clamp(0, 1)
    disps = (0.5 + 0.4 * torch.sin(0.03 * xx + ph[..., 0]) * torch.cos(0.05 * yy)) + 0.01 * torch.randn((N, H, W), generator=gen, device=dev)
    return rgbs.contiguous(), gts.contiguous(), disps.contiguous()


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


def stats(ms):
    q = np.percentile(ms, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "p25": round(float(q[0]), 4), "p75": round(float(q[2]), 4), "min": round(float(np.min(ms)), 4),
            "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 120], help="frame counts to time, each at 400 x 400")
    ap.add_argument("--no-profiler", action="store_true", help="leave torch.profiler's kernel count out (for a run under rocprofv3, which traces the kernels itself)")
    ap.add_argument("--no-host", action="store_true", help="leave route (c) out")
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import frames as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames: needs a GPU")
    import frames_ref as R
    dev = torch.device("cuda")
    lut_np = np.stack([np.random.RandomState(77 + c).permutation(256) for c in range(3)], -1).astype(np.uint8)
    lut = torch.as_tensor(lut_np, device=dev)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    fns = {}

    def emit():
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    def once(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    for N in a.frames:
        key = f"{N}x{H}x{W}"
        px = N * H * W
        try:
            rgbs, gts, disps = inputs(N, H, W, dev)
        except torch.OutOfMemoryError:
            res["shapes"][key] = {"skipped": "out of device memory"}
            continue

        def new(rgbs=rgbs, gts=gts, disps=disps):
            return F.depth_images(disps, invert=True, scope="all", colormap=lut), F.error_maps(rgbs, gts, colormap=lut), F.video_frames(rgbs)

        def comp(rgbs=rgbs, gts=gts, disps=disps):
            return composed(rgbs, gts, disps, lut)

        n, c = new(), comp()
        r = {"bytes": px * ((2 * 4 + 3) + (2 * 24 + 3) + (2 * 12 + 3)),
             "bytes_differing_new_vs_composed": {k: int((x != y).sum()) for k, x, y in zip(("depth", "err", "video"), n, c)}}
        for _ in range(10):
            new()
            comp()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(a.reps):                          # alternating: both routes see the same neighbours on the machine
            ta.append(once(new))
            tb.append(once(comp))
        r["new_ms"], r["composed_ms"] = stats(ta), stats(tb)
        r["speedup_new_over_composed"] = round(r["composed_ms"]["median"] / r["new_ms"]["median"], 2)
        r["new_gbps"] = round(r["bytes"] / (r["new_ms"]["median"] * 1e-3) / 1e9, 1)
        ts, h = [], None
        for i in range(0 if a.no_host else 4):           # the first run warms the host buffers and is dropped
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = host(rgbs, gts, disps, lut_np, R)
            ts.append((time.perf_counter() - t0) * 1e3)
        if h is not None:
            r["host_ms"] = [round(t, 2) for t in ts[1:]]
            r["bytes_differing_new_vs_host"] = {k: int((x.cpu().numpy() != y).sum()) for k, x, y in zip(("depth", "err", "video"), n, h)}
        r["device_to_host_bytes"] = {"new_uint8_pictures": px * 9, "host_float32_frames": px * 28}
        res["shapes"][key] = r
        fns[key] = (new, comp)
        del n, c, h
        emit()                                           # the times are on disk before the next shape and the profiler start
    for key, (new, comp) in ({} if a.no_profiler else fns).items():
        res["shapes"][key]["device_kernels"] = {"new": kernel_count(new), "composed": kernel_count(comp)}
    print(emit())


if __name__ == "__main__":
    main()
