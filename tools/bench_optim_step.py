#!/usr/bin/env python
"""The optimizer step at the blurfactory model's sizes (tools/bench_train_step.py `run`: cv, fv), GPU only: what a training loop does
between loss.backward() and the next forward, two ways, timed back to back in one process, alternating:

    torch    torch.optim.Adam(fused=True).step(), the fills of the in-place gradient buffers, evd_voxel_load_grids for both levels
    library  ONE evdeblurnerf_amd.optim.Adam(model=..., zero_grads=True).step(): Adam, the levels' float32 / float16 grid copies and
             the clearing of the gradients in one pass

Bytes are counted from the shapes (reads + writes the algorithm needs) and set against the 6.3 TB/s copy ceiling of the MI355X.
    python tools/bench_optim_step.py [--reps 30] [--out profiles/optim_step_bench.json]"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from evdeblurnerf_amd import optim as O, weights as W  # noqa: E402
from evdeblurnerf_amd.renderer import NeRFAll  # noqa: E402

AABB = ([-1.5, -1.5, -1.0], [1.5, 1.5, 1.0])
COPY_CEILING = 6.3e12


def build(cv, fv):
    gc, gf = W.pdrf_grid_size(AABB[0], AABB[1], cv), W.pdrf_grid_size(AABB[0], AABB[1], fv)
    sd = dict(W.prefixed(W.make_pdrf_state_dict(31, gc, input_ch=95, hidden_dim=64, geo_feat_dim=15), "mlp_coarse"))
    sd.update(W.prefixed(W.make_pdrf_state_dict(32, gf, input_ch=127, hidden_dim=256, geo_feat_dim=128), "mlp_fine"))
    args = SimpleNamespace(mode="c2f", multires=10, multires_views=4, use_viewdirs=True, N_importance=64, kernel_type="RBK", kernel_use_awp=False,
                           rgb_activate="sigmoid", sigma_activate="relu", bounding_box=AABB, coarse_num_layers=2, coarse_num_layers_color=3,
                           coarse_hidden_dim=64, coarse_hidden_dim_color=64, coarse_app_dim=32, coarse_app_n_comp=[64, 16, 16], coarse_n_voxels=cv,
                           kernel_feat_cnl=15, fine_num_layers=2, fine_num_layers_color=3, fine_hidden_dim=256, fine_hidden_dim_color=256,
                           fine_geo_feat_dim=128, fine_app_dim=32, fine_app_n_comp=[64, 16, 16], fine_n_voxels=fv)
    return NeRFAll(args, sd, precision="f16").enable_training(sd, grads_in_place=True).train()


def attach_gradients(model):
    """the in-place mode's persistent buffers with every leaf's .grad a slice of them, as a backward leaves them; -> the buffers"""
    bufs = []
    for lv in model._levels:
        bufs.append(lv.attach_grads())
        buf, off = lv.net._grid_grad_flat, 0
        for t in lv.grids.values():
            t.grad = buf[off:off + t.numel()].view(t.shape)
            off += t.numel()
        bufs.append(buf)
    for b in bufs:
        b.normal_(0, 1e-3)
    return bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--coarse-voxels", type=int, default=16777248)
    ap.add_argument("--fine-voxels", type=int, default=134217984)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step needs a GPU")
    model = build(a.coarse_voxels, a.fine_voxels)
    params = model.parameters()
    bufs = attach_gradients(model)
    t_opt = torch.optim.Adam(params, lr=5e-4, fused=True)
    l_opt = O.Adam(params, lr=5e-4, model=model, zero_grads=True)
    levels = [(lv.net, list(lv.grids.values())) for lv in model._levels]

    def torch_sequence():
        t_opt.step()
        for b in bufs:
            b.zero_()
        for net, grids in levels:
            net.load_grids(grids)

    def library_step():
        l_opt.step()

    n = sum(p.numel() for p in params)
    n_grid = sum(t.numel() for _, grids in levels for t in grids)
    n_f16 = sum(t.numel() for _, grids in levels for t in grids[:6])
    n_buf = sum(b.numel() for b in bufs)
    # reads + writes: Adam moves p, g, m, v in and p, m, v out; a fill writes; the grid load reads float32 and writes float32 + float16
    bytes_torch = 28 * n + 4 * n_buf + (8 * n_grid + 2 * n_f16)
    bytes_lib = 28 * n + 4 * n + (4 * n_grid + 2 * n_f16)
    ms = {"torch": [], "library": []}
    for fn in (torch_sequence, library_step) * 3:                # warm-up of both (state creation, table upload)
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn in (("torch", torch_sequence), ("library", library_step)):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}
    res = {"device_name": torch.cuda.get_device_name(0), "reps": a.reps, "parameters": n, "grid_elements": n_grid, "gradient_buffer_elements": n_buf,
           "tensors": len(params)}
    for name, nbytes in (("torch", bytes_torch), ("library", bytes_lib)):
        s = stat(ms[name])
        s["bytes"] = int(nbytes)
        s["achieved_TB_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e12, 3)
        s["share_of_copy_ceiling"] = round(nbytes / (s["median_ms"] * 1e-3) / COPY_CEILING, 3)
        res[name] = s
    res["torch"]["what"] = "torch.optim.Adam(fused=True).step() + fills of the gradient buffers + evd_voxel_load_grids of both levels"
    res["library"]["what"] = "optim.Adam(model=..., zero_grads=True).step()"
    res["library_over_torch"] = round(res["library"]["median_ms"] / res["torch"]["median_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
