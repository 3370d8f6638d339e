"""Golden G41: the reference's VoxelNeRFBase (networks/pdrf/voxnerf.py) in float64 on the CPU, for the level shapes of the generic PDRF
level's tests (tests/voxel_generic_ref.py CASES): raw and geo rows at seeded samples, and per parameter tensor the gradient's norm, seeded projection and
pinned elements (G18's form) of sum(raw * d raw).  Data only; tests/test_voxel_generic_ref.py holds the float64 restatement to it.

The class's own forward composites raw before returning it, so its per-sample part (voxnerf.py:210-221,240-254) is run here on the
class's OWN layers (sigma_net, color_net) and the reference's embedder.

    python tools/gen_golden_voxel_generic.py
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
import torch.nn.functional as F  # noqa: E402

import voxel_generic_ref as G  # noqa: E402
from torch_restatement import grad_elements, grad_summary  # noqa: E402


def main():
    from networks.embedding import get_embedder
    from networks.pdrf.voxnerf import VoxelNeRFSampleFeatures
    out = {}
    for ci, (name, (HD, Gd, FT, NS, NC, L, Lv, bias, R, S)) in enumerate(G.CASES.items()):
        sd = G.case_state_dict(name)
        aabb = (torch.tensor(G.AABB[0], dtype=torch.float32), torch.tensor(G.AABB[1], dtype=torch.float32))
        net = VoxelNeRFSampleFeatures(aabb, num_layers=NS, hidden_dim=HD, geo_feat_dim=Gd, num_layers_color=NC, add_bias_color=bias,
                                      input_ch=FT + 3 * (1 + 2 * L), input_ch_views=3 * (1 + 2 * Lv), n_voxels=G.NVOX)
        ref_import.load_np_state_dict(net, sd)
        net = net.double()
        a = G.case_inputs(name)
        pts = torch.tensor(a["pts"], dtype=torch.float64)
        viewdirs = torch.tensor(a["vd"], dtype=torch.float64)
        fts = torch.tensor(a["fts"], dtype=torch.float64)
        pts_embed, _ = get_embedder(L)
        dirs_embed, _ = get_embedder(Lv)
        # the per-sample part (composite_feature=False) on the class's own layers, every sample a row
        n = R * S
        x = torch.cat([fts.reshape(n, FT), pts_embed(pts.reshape(n, 3))], -1)
        for l, lin in enumerate(net.sigma_net):
            x = lin(x) if l == NS - 1 else F.relu(lin(x))
        geo = x[:, 1:]
        c = torch.cat([geo, dirs_embed(viewdirs[:, None].expand(R, S, 3).reshape(n, 3))], -1)
        for l, lin in enumerate(net.color_net):
            c = lin(c) if l == NC - 1 else F.relu(lin(c))
        raw = torch.cat([x[:, :1], torch.sigmoid(c)], -1)
        loss = (raw * torch.tensor(a["d_raw"], dtype=torch.float64).reshape(-1, 4)).sum()
        params = [(k, p) for k, p in net.named_parameters() if k.startswith(("sigma_net.", "color_net."))]
        grads = torch.autograd.grad(loss, [p for _, p in params])
        # raw at 256 seeded samples and whole geo rows at 16 of them (all of them where the run has fewer): the file stays small
        rs = np.random.RandomState(5000 + ci)
        si = np.sort(rs.choice(n, size=min(256, n), replace=False))
        out[f"{name}.sample_idx"] = si.astype(np.int32)
        out[f"{name}.raw"] = raw.detach().numpy()[si]
        out[f"{name}.geo"] = geo.detach().numpy()[si[::16]]
        out[f"{name}.names"] = np.array([k for k, _ in params])
        for i, ((key, _), g) in enumerate(zip(params, grads)):
            g = g.detach().numpy()
            sm, _ = grad_summary(g, 7000 + 100 * ci + i)
            idx, val = grad_elements(g, 9000 + 100 * ci + i, k=32)
            out[f"{name}.{key}.summary"] = sm.astype(np.float64)
            out[f"{name}.{key}.elem_idx"] = idx.astype(np.int32)
            out[f"{name}.{key}.elem_val"] = val.astype(np.float64)
    path = os.path.join(ROOT, "tests", "golden", "G41_voxel_generic.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.relpath(path, ROOT)}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
