#!/usr/bin/env python
"""Time the rigid blur kernel network at the shipped shape: R = 1024 rays, P = 10 (num_motion 9 + the origin), n = 34 images, widths 32.

    python tools/bench_rigid_blur.py [--reps 20] [--out profiles/rigid_blur_bench.json]      on the GPU
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_rigid_blur.py --reps 5 --no-profiler      (profiles/rigid_blur_kernel_stats.csv)

In one run on one box, HIP events around each repetition, 5 warm-up calls, the median of --reps, for
  (a) device   evdeblurnerf_amd.blurmodel.RigidBlurKernel (evd_rigid_blur_forward / _backward)
  (b) torch    tools/rigid_blur_torch.py: the same function as batched PyTorch ops under autograd
each as forward alone and forward + backward of a projected sum (the projection's own ops are inside both timings).  Launches: a
TorchDispatchMode counts, by forward and backward, every aten op with device work that is not a view or an allocation (the method of
tools/trace_aten_kernels.py), and torch.profiler counts the device kernels of one forward + backward after the warm-up -- the library's
own launches appear there as evd::k_rigid_blur_*.  Prints one JSON line; --out also writes it to a file."""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R, P, N_IMG, C = 1024, 10, 34, 32
NO_KERNEL = ("view", "reshape", "empty", "as_strided", "slice", "select", "expand", "unsqueeze", "squeeze", "transpose", "permute", "detach", "alias",
             "t.default", "split", "unbind", "narrow", "_unsafe_view", "set_", "resize_", "is_", "size", "stride", "numel", "sym_", "lift_fresh",
             "_local_scalar_dense", "unfold", "chunk", "record_stream", "_has_", "item")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-profiler", action="store_true", help="leave torch.profiler's kernel count out (for a run under rocprofv3, which traces the kernels itself)")
    a = ap.parse_args()
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    from rigid_blur_torch import TorchRigidBlur
    dev = "cuda"
    torch.manual_seed(37)
    device_mod = RigidBlurKernel(N_IMG, embed_dim=C, embed_init="normal", num_motion=P - 1).to(dev)
    torch_mod = TorchRigidBlur(N_IMG, embed_dim=C, num_motion=P - 1).to(dev)
    torch_mod.load_state_dict(device_mod.state_dict())
    rays = torch.as_tensor(W.synthetic_rays(1, R), device=dev)
    info = {"images_idx": torch.randint(0, N_IMG, (R, 1), device=dev)}
    proj = [torch.randn((R, P, 3, 2), device=dev), torch.randn((R, P), device=dev), torch.randn((R, C), device=dev)]

    def forward(mod):
        new_rays, weight, _, extras = mod(400, 400, None, rays, info, return_img_embed=True)
        return (new_rays * proj[0]).sum() + (weight * proj[1]).sum() + (extras["img_embed"] * proj[2]).sum()

    def both(mod):
        mod.zero_grad(set_to_none=True)
        forward(mod).backward()

    class Watch(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.n = collections.Counter()
            self.phase = None

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func).replace("aten.", "")
            ts = [t for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)]
            if self.phase and any(t.is_cuda for t in ts) and not any(k in name for k in NO_KERNEL):
                self.n[(self.phase, name)] += 1
            return out

    def aten_ops(mod):
        """aten ops with device work of the MODULE's forward and of the backward behind its outputs (the projection stays outside)"""
        torch.autograd.set_multithreading_enabled(False)
        w = Watch()
        with w:
            mod.zero_grad(set_to_none=True)
            w.phase = "forward"
            new_rays, weight, _, extras = mod(400, 400, None, rays, info, return_img_embed=True)
            w.phase = None
            outs = [new_rays, weight, extras["img_embed"]]
            w.phase = "backward"
            torch.autograd.backward(outs, proj)
            w.phase = None
        per = {ph: {k[1]: v for k, v in w.n.items() if k[0] == ph} for ph in ("forward", "backward")}
        return {ph: {"total": sum(d.values()), "ops": d} for ph, d in per.items()}

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
            new_rays, weight, _, extras = mod(400, 400, None, rays, info, return_img_embed=True)
            torch.autograd.backward([new_rays, weight, extras["img_embed"]], proj)
            torch.cuda.synchronize()
        ka = [e for e in prof.key_averages() if e.device_time_total > 0]
        lib = {e.key.split("(")[0]: e.count for e in ka if "k_rigid_blur" in e.key}
        return {"device_kernels": int(sum(e.count for e in ka)), "device_time_us": round(sum(e.device_time_total for e in ka), 1), "library": lib}

    with torch.no_grad():
        o_d = device_mod(400, 400, None, rays, info)
        o_t = torch_mod(400, 400, None, rays, info)
    res = {"shape": {"R": R, "P": P, "n_img": N_IMG, "C": C, "widths": 32}, "reps": a.reps,
           "max_abs_device_minus_torch": {"new_rays": float((o_d[0] - o_t[0]).abs().max()), "weight": float((o_d[1] - o_t[1]).abs().max())}}
    for name, mod in (("device", device_mod), ("torch", torch_mod)):
        res[name] = {"forward_ms": timed(lambda: forward(mod)), "forward_backward_ms": timed(lambda: both(mod)), "aten_ops_with_device_work": aten_ops(mod)}
        if not a.no_profiler:
            res[name]["one_forward_backward"] = kernels(mod)
    res["speedup_forward_backward"] = round(res["torch"]["forward_backward_ms"]["median"] / res["device"]["forward_backward_ms"]["median"], 2)
    res["device_name"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
