"""Bandwidth of evd_raw2outputs_feat_bwd (the feature-composite backward of a composite_feature level) next to the C = 4 backward
(evd_raw2outputs_bwd_rays), R = 2^17, S = 64, G = 15: hipEvent medians over 30 launches after 5.  python tools/bench_composite_feat_bwd.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from evdeblurnerf_amd import _lib as L
R, S, G = 1 << 17, 64, 15
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
raw = torch.randn((R, S, 4), generator=g, device=dev); rows = torch.randn((R, S, G), generator=g, device=dev)
z = torch.sort(2 + 4 * torch.rand((R, S), generator=g, device=dev), -1)[0].contiguous(); rd = torch.randn((R, 3), generator=g, device=dev)
gf, gm, gd, ga, gw = (torch.randn(s, generator=g, device=dev) for s in ((R, G), (R, 3), (R,), (R,), (R, S)))
d_raw, d_rows, d_rd = torch.empty_like(raw), torch.empty_like(rows), torch.empty_like(rd)
A = L.ACT
def feat():
    L.check(L.lib().evd_raw2outputs_feat_bwd(L.ptr(raw), 4, 0, L.ptr(rows), G, A["relu"], L.ptr(z), L.ptr(rd), 3, None, A["relu"], 0.0, R, S, L.ptr(gf), L.ptr(gd), L.ptr(ga), L.ptr(gw),
                                             L.ptr(d_raw), L.ptr(d_rows), L.ptr(d_rd), 3, L.stream_ptr()), "feat")
def c4():
    L.check(L.lib().evd_raw2outputs_bwd_rays(L.ptr(raw), L.ptr(z), L.ptr(rd), 3, R, S, 4, 0, 1, 3, A["relu"], A["relu"], 0, 0.0, None, L.ptr(gm), L.ptr(gd), L.ptr(ga), L.ptr(gw),
                                             L.ptr(d_raw), L.ptr(d_rd), 3, L.stream_ptr()), "c4")
def med(fn, n=30, warm=5):
    for _ in range(warm): fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))
tf, tc = med(feat), med(c4)
bf = R * S * (8 * G + 24) + R * S * 16          # rows in + d_rows out + z, g_w, sigma (S (8 G + 24) B per ray) + the [R, S, 4] d_raw written
bf_issue = R * S * (8 * G + 24)
bc = R * S * (16 + 4 + 4 + 16)                   # raw, z, g_w in, d_raw out
print(f"feat bwd R={R} S={S} G={G}: median {tf[0]:.3f} ms (min {tf[1]:.3f}, max {tf[2]:.3f}); {bf_issue / tf[0] / 1e6:.0f} GB/s on S (8 G + 24) B per ray, "
      f"{bf / tf[0] / 1e6:.0f} GB/s counting the [R, S, 4] d_raw it also writes")
print(f"C=4 bwd  R={R} S={S}: median {tc[0]:.3f} ms (min {tc[1]:.3f}, max {tc[2]:.3f}); {bc / tc[0] / 1e6:.0f} GB/s on S 40 B per ray")
