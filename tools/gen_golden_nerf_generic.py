"""Golden G40: the reference's NeRF class (networks/nerf.py) in float64 on the CPU, for the six networks of the generic training path's
tests (tests/nerf_generic_ref.py CASES): raw, and per parameter tensor the gradient's norm, seeded projection and 256 pinned elements
(G18's form) of sum(raw * d raw).  Data only; tests/test_nerf_generic_ref.py holds the float64 restatement to it.

    python tools/gen_golden_nerf_generic.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402

ref_import.install()

import torch  # noqa: E402

import nerf_generic_ref as G  # noqa: E402
from torch_restatement import grad_elements, grad_summary  # noqa: E402


def main():
    from networks.embedding import get_embedder
    from networks.nerf import NeRF
    out = {}
    for ci, (name, (D, Wd, L, Lv, skip, R, S, _)) in enumerate(G.CASES.items()):
        sd = G.case_state_dict(name)
        net = NeRF(D=D, W=Wd, input_ch=3 * (1 + 2 * L), input_ch_views=3 * (1 + 2 * Lv), output_ch=4, skips=[] if skip is None else [skip],
                   use_viewdirs=True, rgb_add_bias=True)
        ref_import.load_np_state_dict(net, sd)
        net = net.double()
        rb, z, d_raw = G.case_inputs(name)
        pts, dirs = G.positions(rb, z)
        e_pts, _ = get_embedder(L)
        e_dirs, _ = get_embedder(Lv)
        raw, _ = net.eval(torch.cat([e_pts(pts), e_dirs(dirs)], -1))
        loss = (raw * torch.tensor(d_raw, dtype=torch.float64).reshape(-1, 4)).sum()
        params = list(net.named_parameters())
        grads = torch.autograd.grad(loss, [p for _, p in params])
        out[f"{name}.raw"] = raw.detach().numpy()
        for i, ((key, _), g) in enumerate(zip(params, grads)):
            g = g.detach().numpy()
            sm, _ = grad_summary(g, 7000 + 100 * ci + i)
            idx, val = grad_elements(g, 9000 + 100 * ci + i, k=128)          # the 128 largest elements + 128 seeded random ones
            out[f"{name}.{key}.summary"] = sm.astype(np.float64)
            out[f"{name}.{key}.elem_idx"] = idx.astype(np.int32)
            out[f"{name}.{key}.elem_val"] = val.astype(np.float64)
    path = os.path.join(ROOT, "tests", "golden", "G40_nerf_generic_grads.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.relpath(path, ROOT)}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
