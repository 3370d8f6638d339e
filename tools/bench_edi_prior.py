#!/usr/bin/env python
"""Time the EDI prior table at the DAVIS shape: 8 images, 260 x 346, steps 9, 2 M events.

    python tools/bench_edi_prior.py [--reps 20] [--out profiles/edi_prior_bench.json]      on the GPU
    python tools/bench_edi_prior.py --reference                                            on a machine that holds the reference (CPU)

On the GPU, in one run, HIP events around each repetition, 3 warm-up calls, the median of --reps:
  (a) new          edi.compute_edi_prior (evd_edi_prior: one call, no read-back)
  (b) composed     what a user had to write from the two older entries: torch.searchsorted twice, per image and window a slice, the
                   coordinate gather, evd_edi_bii_image, the channel broadcast, then evd_edi_deblur per image
  (c) new, no events   the same call on an empty event table: windows + clearing + deblur; (a) - (c) is taken as the splat's time, and
                   the atomic bytes per second are (number of taps that land) x 8 bytes / that time
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

H, W, STEPS, N_IMG, N_EV, CPOS, CNEG = 260, 346, 9, 8, 2_000_000, 0.2, 0.25


def inputs():
    rs = np.random.RandomState(36)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cx, cy = gx.reshape(-1), gy.reshape(-1)
    i2c = np.stack([cx + 0.31 * np.sin(0.04 * cy) + 0.45, cy + 0.27 * np.cos(0.03 * cx) + 0.35], -1).astype(np.float32).astype(np.float64)
    ids = rs.randint(0, H * W, N_EV)
    start = 500_000.0 + 12_000.0 * np.arange(N_IMG)
    end = start + 10_000.0
    t = np.sort(rs.randint(int(start[0]) - 2_000, int(end[-1]) + 2_000, N_EV)).astype(np.float64)
    p = np.where(rs.rand(N_EV) < 0.5, 1.0, -1.0)
    events = np.stack([ids.astype(np.float64), t, p, np.zeros(N_EV)], -1)
    images = rs.uniform(0.02, 1.0, (N_IMG, H, W, 3)).astype(np.float32)
    return events, i2c, start, end, images


def taps_landed(events, i2c, start, end):
    """taps the splat adds (one 8-byte atomic each): per window of every image, the in-frame floor / ceil combinations of its events"""
    n = 0
    t = events[:, 1]
    for a, b in zip(start, end):
        bd = np.linspace(a, b, STEPS)
        left, right = np.searchsorted(t, bd, side="left"), np.searchsorted(t, bd, side="right")
        for j in range(STEPS - 1):
            xy = i2c[events[left[j]:right[j + 1], 0].astype(np.int64)]
            fx, fy = np.floor(xy[:, 0]), np.floor(xy[:, 1])
            nx = ((fx >= 0) & (fx < W)).astype(np.int64) + ((xy[:, 0] > fx) & (fx + 1 >= 0) & (fx + 1 < W))
            ny = ((fy >= 0) & (fy < H)).astype(np.int64) + ((xy[:, 1] > fy) & (fy + 1 >= 0) & (fy + 1 < H))
            n += int((nx * ny).sum())
    return n


def reference_seconds(events, i2c, start, end, images):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_import
    ref_import.install()
    import types
    import torch
    import data.loader_events as LE
    fake = types.SimpleNamespace(images_tms_start=start, images_tms_end=end, events=torch.from_numpy(events), id_to_coords=torch.from_numpy(i2c), device="cpu")
    t0 = time.perf_counter()
    LE.LLFFEventsDataset.compute_edi_prior(fake, np.arange(N_IMG), torch.from_numpy(images), STEPS, CPOS, CNEG)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", action="store_true", help="time the reference's compute_edi_prior on the CPU instead (needs the reference)")
    a = ap.parse_args()
    events, i2c, start, end, images = inputs()
    res = {"shape": {"n_img": N_IMG, "h": H, "w": W, "steps": STEPS, "events": N_EV}}
    if a.reference:
        res["reference_cpu_s"] = [round(reference_seconds(events, i2c, start, end, images), 3) for _ in range(3)]
    else:
        import torch
        from evdeblurnerf_amd import edi
        dev = "cuda"
        ev, ic, img = torch.as_tensor(events, device=dev), torch.as_tensor(i2c, device=dev), torch.as_tensor(images, device=dev)
        ev0 = ev[:0].contiguous()
        xy32 = ic.to(torch.float32)

        def new():
            return edi.compute_edi_prior(ev, ic, start, end, img, STEPS, CPOS, CNEG, check=False)

        def new_no_events():
            return edi.compute_edi_prior(ev0, ic, start, end, img, STEPS, CPOS, CNEG, check=False)

        def composed():
            bd = torch.as_tensor(np.concatenate([np.linspace(s, e, STEPS) for s, e in zip(start, end)]), device=dev)
            tms = ev[:, 1].contiguous()
            left = torch.searchsorted(tms, bd).reshape(N_IMG, STEPS).tolist()
            right = torch.searchsorted(tms, bd, side="right").reshape(N_IMG, STEPS).tolist()
            out = []
            for i in range(N_IMG):
                bii = []
                for j in range(STEPS - 1):
                    e = ev[left[i][j]:right[i][j + 1]]
                    c = xy32[e[:, 0].long()]
                    b = edi.brightness_increment_image(c[:, 0], c[:, 1], e[:, 2], W, H, CPOS, CNEG)
                    bii.append(b[..., None].expand(H, W, 3))
                out.append(edi.deblur_double_integral(img[i], torch.stack(bii)))
            return torch.stack(out)

        def timed(fn):
            for _ in range(3):
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
            return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

        worst = float((new() - composed()).abs().max())
        taps = taps_landed(events, i2c, start, end)
        for name, fn in (("new", new), ("composed", composed), ("new_no_events", new_no_events)):
            med, lo, hi = timed(fn)
            res[name + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        splat_ms = res["new_ms"]["median"] - res["new_no_events_ms"]["median"]
        res.update({"reps": a.reps, "taps": taps, "atomic_bytes": taps * 8, "splat_ms_by_difference": round(splat_ms, 4),
                    "atomic_GB_per_s": round(taps * 8 / (splat_ms * 1e-3) / 1e9, 2) if splat_ms > 0 else None,
                    "speedup_new_over_composed": round(res["composed_ms"]["median"] / res["new_ms"]["median"], 2),
                    "max_abs_new_minus_composed": worst, "device": torch.cuda.get_device_name(0)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
