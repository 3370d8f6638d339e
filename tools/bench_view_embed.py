#!/usr/bin/env python
"""Time kernel_img_embed_type 'param_mlp' in front of both blur kernel networks at the shipped shape: R = 1024 rays, n = 34 images,
E = W = 32, D = 4 (skips=[4], inert), RigidBlurKernel with M = 9 and SparseBlurKernel (DSK) with 5 points per ray.

    python tools/bench_view_embed.py [--reps 20] [--out profiles/view_embed_mlp_bench.json]      on the GPU
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_view_embed.py --reps 5 --no-profiler    (profiles/view_embed_mlp_kernel_stats.csv)

In one process on one box, HIP events around each repetition, 5 warm-up calls, the median of --reps, forward + backward of a projected sum:
  (a) table    blurmodel.ViewEmbeddingMLP: evd_view_embed_mlp_forward / _backward on n rows, the blur kernel gathers from the table by ids
  (b) per_ray  tools/view_embed_torch.py handed to the same kernel module as `view_embed`: the MLP as PyTorch ops on R rows and the
               kernel's per-ray (x) form -- the route a caller had before the table kernels
Both hold the same parameters.  torch.profiler counts the device kernels of one forward + backward after the warm-up.  Prints one JSON
line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R, N_IMG, E, WD, D, SKIPS, M, PTS = 1024, 34, 32, 32, 4, [4], 9, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-profiler", action="store_true", help="leave torch.profiler's kernel count out (for a run under rocprofv3, which traces the kernels itself)")
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel, SparseBlurKernel, ViewEmbeddingMLP
    from view_embed_torch import TorchViewEmbeddingMLP
    dev = "cuda"
    torch.manual_seed(40)
    rays = torch.as_tensor(W.synthetic_rays(1, R), device=dev)
    ids = torch.randint(0, N_IMG, (R, 1), device=dev)
    kmat = np.array([[350, 0, 200], [0, 350, 200], [0, 0, 1]], np.float32)
    info = {"images_idx": ids, "rays_x": torch.randint(0, 400, (R, 1), device=dev).float(), "rays_y": torch.randint(0, 400, (R, 1), device=dev).float(),
            "poses": torch.randn((R, 3, 4), device=dev)}
    noise = torch.randn((R, PTS, 2), device=dev)

    def modules(kind):
        """the table-route and the per-ray-route module of one kernel type, with the same parameters"""
        table_ve = ViewEmbeddingMLP(D, WD, SKIPS, N_IMG, E, init_params="normal")
        ray_ve = TorchViewEmbeddingMLP(D, WD, SKIPS, N_IMG, E)
        if kind == "rigid":
            mods = [RigidBlurKernel(N_IMG, num_motion=M, view_embed=ve) for ve in (table_ve, ray_ve)]
        else:
            mods = [SparseBlurKernel(N_IMG, PTS, 10, "DSK", view_embed=ve, view_embed_cnl=WD) for ve in (table_ve, ray_ve)]
        mods[1].load_state_dict(mods[0].state_dict())
        return [m.to(dev) for m in mods]

    def outputs(kind, mod):
        if kind == "rigid":
            new_rays, weight, _, extras = mod(400, 400, None, rays, info, return_img_embed=True)
            return [new_rays, weight, extras["img_embed"]]
        new_rays, weight, align, extras = mod(400, 400, kmat, None, info, return_img_embed=True, noise=noise)
        return [new_rays, weight, extras["img_embed"], align]

    def timed(fn):
        for _ in range(5):
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

    res = {"shape": {"R": R, "n_img": N_IMG, "E": E, "W": WD, "D": D, "skips": SKIPS, "M": M, "num_pt": PTS}, "reps": a.reps}
    for kind in ("rigid", "sparse"):
        mods = dict(zip(("table", "per_ray"), modules(kind)))
        with torch.no_grad():
            o = {k: outputs(kind, m) for k, m in mods.items()}
        proj = [torch.randn_like(t) for t in o["table"]]
        res[kind] = {"max_abs_table_minus_per_ray": {n: float((x - y).abs().max()) for n, x, y in zip(("new_rays", "weight", "img_embed"), o["table"], o["per_ray"])}}

        def both(mod):
            mod.zero_grad(set_to_none=True)
            torch.autograd.backward(outputs(kind, mod), proj)

        for route, mod in mods.items():
            r = {"forward_backward_ms": timed(lambda: both(mod))}
            if not a.no_profiler:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    both(mod)
                    torch.cuda.synchronize()
                ka = [e for e in prof.key_averages() if e.device_time_total > 0]
                r["one_forward_backward"] = {"device_kernels": int(sum(e.count for e in ka)), "device_time_us": round(sum(e.device_time_total for e in ka), 1),
                                             "library": {e.key.split("(")[0]: e.count for e in ka if "evd::k_" in e.key}}
            res[kind][route] = r
        res[kind]["per_ray_over_table"] = round(res[kind]["per_ray"]["forward_backward_ms"]["median"] / res[kind]["table"]["forward_backward_ms"]["median"], 2)
    res["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
