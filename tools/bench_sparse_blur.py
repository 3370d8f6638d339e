#!/usr/bin/env python
"""The sparse blur kernel network (BlurModel of networks/pdrf/blurmodel.py, kernel_type DSK) at the options.py defaults, 1024 rays x 5 points,
34 images: forward and forward + backward of

  (a) device   evdeblurnerf_amd.blurmodel.SparseBlurKernel (evd_sparse_blur_forward / _backward)
  (b) torch    tools/sparse_blur_torch.py: the same function as batched float32 PyTorch ops under autograd

    python tools/bench_sparse_blur.py [--reps 20] [--out profiles/sparse_blur_bench.json]      on the GPU

Median of --reps calls after 5 warm-up calls, HIP events around each call.  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R, P, N_IMG, C = 1024, 5, 34, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.blurmodel import SparseBlurKernel
    from sparse_blur_torch import TorchSparseBlur
    dev = "cuda"
    torch.manual_seed(39)
    device_mod = SparseBlurKernel(N_IMG, P, 10, "DSK", embed_init="normal").to(dev)
    torch_mod = TorchSparseBlur(N_IMG, P, 10, "DSK").to(dev)
    torch_mod.load_state_dict(device_mod.state_dict())
    K = W.synthetic_camera()
    info = {"images_idx": torch.randint(0, N_IMG, (R, 1), device=dev), "rays_x": torch.randint(0, 400, (R, 1), device=dev).float() + 0.5,
            "rays_y": torch.randint(0, 400, (R, 1), device=dev).float() + 0.5, "poses": torch.randn((R, 3, 4), device=dev)}
    noise = torch.randn((R, P, 2), device=dev)
    proj = [torch.randn((R, P, 3, 2), device=dev), torch.randn((R, P), device=dev), torch.randn((R, C), device=dev)]

    def forward(mod):
        new_rays, weight, align, extras = mod(400, 400, K, None, info, return_img_embed=True, noise=noise)
        return (new_rays * proj[0]).sum() + (weight * proj[1]).sum() + (extras["img_embed"] * proj[2]).sum() + 0.1 * align

    def both(mod):
        mod.zero_grad(set_to_none=True)
        forward(mod).backward()

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

    def kernels(mod):
        from torch.profiler import ProfilerActivity, profile
        both(mod)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            mod.zero_grad(set_to_none=True)
            new_rays, weight, align, extras = mod(400, 400, K, None, info, return_img_embed=True, noise=noise)
            torch.autograd.backward([new_rays, weight, extras["img_embed"], align], proj + [torch.ones((), device=dev)])
            torch.cuda.synchronize()
        ka = [e for e in prof.key_averages() if e.device_time_total > 0]
        lib = {e.key.split("(")[0]: round(e.device_time_total / e.count, 1) for e in ka if "k_sparse_blur" in e.key}
        return {"device_kernels": int(sum(e.count for e in ka)), "device_time_us": round(sum(e.device_time_total for e in ka), 1), "library_us_per_launch": lib}

    with torch.no_grad():
        o_d = device_mod(400, 400, K, None, info, noise=noise)
        o_t = torch_mod(400, 400, K, None, info, noise=noise)
    res = {"shape": {"R": R, "P": P, "n_img": N_IMG, "C": C, "num_hidden": 3, "num_wide": 64}, "reps": a.reps,
           "max_abs_device_minus_torch": {"new_rays": float((o_d[0] - o_t[0]).abs().max()), "weight": float((o_d[1] - o_t[1]).abs().max()),
                                          "align": float((o_d[2] - o_t[2]).abs())}}
    for name, mod in (("device", device_mod), ("torch", torch_mod)):
        res[name] = {"forward_ms": timed(lambda: forward(mod)), "forward_backward_ms": timed(lambda: both(mod)), "one_forward_backward": kernels(mod)}
    res["speedup_forward_backward"] = round(res["torch"]["forward_backward_ms"]["median"] / res["device"]["forward_backward_ms"]["median"], 2)
    res["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
