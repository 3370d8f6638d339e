"""Forward + backward time of one NeRF.mlp_train call on the generic training path (EVD_PREC_F16X3) at R = 2048, S = 64 (2^17 samples),
alternated in the same process with the same network written as float32 torch.nn.Linear layers + encodings on the GPU (the reference's
own operations).  4 x 64 (6, 2) and 8 x 256 (6, 2); device events, warmed up, every timed window at least half a second.

    python tools/bench_nerf_generic_train.py [--out profiles/nerf_generic_train_bench.json]
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
from evdeblurnerf_amd.nerf import NeRF  # noqa: E402


def embed(x, L):
    out = [x]
    for k in range(L):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, -1)


class TorchNet(torch.nn.Module):
    """networks/nerf.py:131-162 with nn.Linear layers, float32"""

    def __init__(self, sd, D, L, Lv, skip):
        super().__init__()
        self.D, self.L, self.Lv, self.skip = D, L, Lv, skip

        def lin(key):
            w = torch.tensor(sd[key + ".weight"])
            m = torch.nn.Linear(w.shape[1], w.shape[0])
            m.weight.data.copy_(w)
            m.bias.data.copy_(torch.tensor(sd[key + ".bias"]))
            return m
        self.pts = torch.nn.ModuleList([lin(f"pts_linears.{l}") for l in range(D)])
        self.views, self.feature, self.alpha, self.rgb = lin("views_linears.0"), lin("feature_linear"), lin("alpha_linear"), lin("rgb_linear")

    def forward(self, rb, z):
        S = z.shape[1]
        pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        dirs = rb[:, None, 8:11].expand(-1, S, -1).reshape(-1, 3)
        pe, ped = embed(pts, self.L), embed(dirs, self.Lv)
        h = pe
        for l in range(self.D):
            h = torch.relu(self.pts[l](h))
            if l == self.skip and l < self.D - 1:
                h = torch.cat([pe, h], -1)
        alpha = self.alpha(h)
        hv = torch.relu(self.views(torch.cat([self.feature(h), ped], -1)))
        return torch.cat([self.rgb(hv), alpha], -1).reshape(z.shape[0], S, 4)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_generic_train_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    R, S, L, Lv = 2048, 64, 6, 2
    rs = np.random.RandomState(1)
    rb_np = np.zeros((R, 11), np.float32)
    rb_np[:, 0:3] = rs.uniform(-0.5, 0.5, (R, 3))
    d = rs.normal(size=(R, 3))
    rb_np[:, 3:6] = rb_np[:, 8:11] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rb_np[:, 7] = 1.0
    rb = torch.tensor(rb_np, device="cuda")
    z = torch.tensor(np.sort(rs.uniform(0.2, 2.0, (R, S)).astype(np.float32), -1), device="cuda")
    wgt = torch.tensor((rs.normal(size=(R, S, 4)) * 1e-2).astype(np.float32), device="cuda")
    result = {"samples": R * S, "R": R, "S": S, "multires": L, "multires_views": Lv, "device": torch.cuda.get_device_name(0), "networks": {}}
    ok = True
    for D, Wd, skip in ((4, 64, None), (8, 256, 4)):
        sd = W.make_nerf_state_dict(7, D, Wd, input_ch=W.pe_dim(L), input_ch_views=W.pe_dim(Lv), skips=() if skip is None else (skip,))
        net = NeRF(sd, D=D, W=Wd, multires=L, multires_views=Lv, skips=() if skip is None else (skip,), precision="f16x3")
        flat = net.flat_params(sd)
        tnet = TorchNet(sd, D, L, Lv, skip).cuda()

        def lib_step():
            flat.grad = None
            (net.mlp_train(flat, rb, z) * wgt).sum().backward()

        def torch_step():
            tnet.zero_grad(set_to_none=True)
            (tnet(rb, z) * wgt).sum().backward()

        for _ in range(3):
            lib_step()
            torch_step()
        torch.cuda.synchronize()
        g_lib = flat.grad.clone()
        g_t = torch.cat([p.grad.reshape(-1) for m in (*tnet.pts, tnet.views, tnet.feature, tnet.alpha, tnet.rgb) for p in (m.weight, m.bias)])
        agree = ((g_lib - g_t).norm() / g_t.norm()).item()
        lib_ms, torch_ms = [], []
        for _ in range(a.repeats):              # alternated: both see the same clocks and neighbours
            lib_ms.append(window(lib_step))
            torch_ms.append(window(torch_step))
        entry = {"library_ms": float(np.median(lib_ms)), "library_ms_all": lib_ms, "torch_f32_ms": float(np.median(torch_ms)), "torch_f32_ms_all": torch_ms,
                 "flat_gradient_rel_l2_vs_torch_f32": agree}
        result["networks"][f"{D}x{Wd}"] = entry
        print(f"{D} x {Wd} ({L}, {Lv}): library {entry['library_ms']:.3f} ms (all {['%.3f' % v for v in lib_ms]}), float32 torch "
              f"{entry['torch_f32_ms']:.3f} ms (all {['%.3f' % v for v in torch_ms]}); gradients agree to {agree:.1e}")
        if D == 4 and not entry["library_ms"] <= entry["torch_f32_ms"]:
            ok = False
    result["4x64_not_slower_than_torch"] = ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"4x64_not_slower_than_torch": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
