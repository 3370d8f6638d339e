"""Forward + backward time of one VoxelNeRFBase.mlp_train call on the generic training path (EVD_PREC_F16X3) at R = 2048, S = 64 (2^17
samples), alternated in the same process with the same level written as float32 torch.nn.Linear layers + encodings on the GPU (the
reference's own operations).  Three shapes of tests/voxel_generic_ref.py: 64 / 7 / 32 with 1 + 1 layers, 128 / 31 / 48 with 3 + 4 (the
class defaults), 256 / 100 / 64 with 2 + 2.  Gradients to the parameters, the sampled features and, through the encodings, pts and
viewdirs.  Device events, warmed up, every timed window at least half a second.

    python tools/bench_voxel_generic_train.py [--out profiles/voxel_generic_train_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from evdeblurnerf_amd import weights as W  # noqa: E402
from evdeblurnerf_amd.voxnerf import VoxelNeRFSampleFeatures  # noqa: E402

AABB, NVOX = W.BLURFACTORY_AABB, 24 ** 3
SHAPES = ((64, 7, 32, 1, 1), (128, 31, 48, 3, 4), (256, 100, 64, 2, 2))     # hidden, geo, features, num_layers, num_layers_color


def embed(x, L):
    out = [x]
    for k in range(L):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, -1)


class TorchLevel(torch.nn.Module):
    """networks/pdrf/voxnerf.py:210-221,240-254 with nn.Linear layers (no biases, as shipped), float32"""

    def __init__(self, sd, NS, NC, L, Lv):
        super().__init__()
        self.L, self.Lv = L, Lv

        def lin(key):
            w = torch.tensor(sd[key + ".weight"])
            m = torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
            m.weight.data.copy_(w)
            return m
        self.sigma = torch.nn.ModuleList([lin(f"sigma_net.{l}") for l in range(NS)])
        self.color = torch.nn.ModuleList([lin(f"color_net.{l}") for l in range(NC)])

    def forward(self, pts, vd, fts):
        R, S = pts.shape[:2]
        h = torch.cat([fts.reshape(R * S, -1), embed(pts.reshape(-1, 3), self.L)], -1)
        for l, m in enumerate(self.sigma):
            h = m(h)
            if l != len(self.sigma) - 1:
                h = torch.relu(h)
        c = torch.cat([h[:, 1:], embed(vd[:, None].expand(R, S, 3).reshape(-1, 3), self.Lv)], -1)
        for l, m in enumerate(self.color):
            c = m(c)
            if l != len(self.color) - 1:
                c = torch.relu(c)
        return torch.cat([h[:, :1], torch.sigmoid(c)], -1).reshape(R, S, 4)


def window(fn, min_seconds=0.5):
    """milliseconds per call over one window of at least min_seconds (device events)"""
    n = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1000.0 * min_seconds:
            return ms / n
        n = max(n + 1, int(n * 1.3 * 1000.0 * min_seconds / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_generic_train_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    R, S, L, Lv = 2048, 64, 10, 4
    rs = np.random.RandomState(1)
    d = rs.normal(size=(R, 3))
    wgt = torch.tensor((rs.normal(size=(R, S, 4)) * 1e-2).astype(np.float32), device="cuda")
    result = {"samples": R * S, "R": R, "S": S, "multires": L, "multires_views": Lv, "device": torch.cuda.get_device_name(0), "levels": {}}
    gsz = W.pdrf_grid_size(AABB[0], AABB[1], NVOX)
    for HD, G, FT, NS, NC in SHAPES:
        sd = W.make_pdrf_state_dict(7, gsz, input_ch=FT + 3 * (1 + 2 * L), num_layers=NS, hidden_dim=HD, geo_feat_dim=G, num_layers_color=NC)
        net = VoxelNeRFSampleFeatures(sd, "", AABB, num_layers=NS, hidden_dim=HD, geo_feat_dim=G, num_layers_color=NC, input_ch=FT + 3 * (1 + 2 * L),
                                      app_dim=32, app_n_comp=(64, 16, 16), n_voxels=NVOX, precision="f16x3")
        flat = net.flat_params(sd)
        tnet = TorchLevel(sd, NS, NC, L, Lv).cuda()
        pts = torch.tensor(rs.uniform(-1, 1, (R, S, 3)).astype(np.float32), device="cuda", requires_grad=True)
        vd = torch.tensor((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32), device="cuda", requires_grad=True)
        fts = torch.tensor((0.3 * rs.normal(size=(R, S, FT))).astype(np.float32), device="cuda", requires_grad=True)
        leaves = (pts, vd, fts)

        def lib_step():
            flat.grad = None
            for t in leaves:
                t.grad = None
            (net.mlp_train(flat, pts, vd, fts, "f16x3") * wgt).sum().backward()

        def torch_step():
            tnet.zero_grad(set_to_none=True)
            for t in leaves:
                t.grad = None
            (tnet(pts, vd, fts) * wgt).sum().backward()

        for _ in range(3):
            lib_step()
            torch_step()
        torch.cuda.synchronize()
        lib_step()
        g_lib = {k: v.clone() for k, v in net.unflatten(flat.grad).items() if k.endswith("weight")}
        torch_step()
        g_t = {f"{n}_net.{l}.weight": m.weight.grad for n, ms in (("sigma", tnet.sigma), ("color", tnet.color)) for l, m in enumerate(ms)}
        agree = max(((g_lib[k] - g_t[k]).norm() / g_t[k].norm()).item() for k in g_t)
        lib_ms, torch_ms = [], []
        for _ in range(a.repeats):              # alternated: both see the same clocks and neighbours
            lib_ms.append(window(lib_step))
            torch_ms.append(window(torch_step))
        entry = {"library_ms": float(np.median(lib_ms)), "library_ms_all": lib_ms, "torch_f32_ms": float(np.median(torch_ms)), "torch_f32_ms_all": torch_ms,
                 "store_MiB": int(net_store_bytes(net, R * S)) / 2 ** 20, "worst_weight_gradient_rel_l2_vs_torch_f32": agree}
        result["levels"][f"{HD}/{G}/{FT} {NS}+{NC}"] = entry
        print(f"{HD} / {G} / {FT}, {NS} + {NC} layers: library {entry['library_ms']:.3f} ms (all {['%.3f' % v for v in lib_ms]}), float32 torch "
              f"{entry['torch_f32_ms']:.3f} ms (all {['%.3f' % v for v in torch_ms]}); store {entry['store_MiB']:.0f} MiB; gradients agree to {agree:.1e}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    return 0


def net_store_bytes(net, nsamp):
    from evdeblurnerf_amd import _lib as L
    return L.lib().evd_voxel_train_store_bytes_prec(net._h, L.PREC["f16x3"], nsamp)


if __name__ == "__main__":
    sys.exit(main())
