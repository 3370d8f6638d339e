"""CPU-only: a torch / float64 restatement of the kernel_type PBE composition (networks/renderer.py:286-378 on voxnerf.py:210-259) reproduces
golden G44 (tools/gen_golden_pbe.py) from the blur kernel's recorded outputs: stage-0 rays -> coarse level with composite_feature (geo rows
-> relu -> composite -> per-ray colour network) -> rgb0 = sum_p weight0 rgb0_pts;  stage-1 rays -> c2f render on the golden's sample
positions, whose coarse colour is again the per-ray network's -> rgb = sum_p weight1 rgb_pts, rgb1 = (rgb0 + sum_p weight1 rgb1_pts) / 2.
This pins the order of operations independently of the kernels.  (The feature map the stage-1 kernel call consumed is behind the recorded
kernel outputs; tests/test_gpu_pbe_train_call.py checks its gradient.)"""
import numpy as np
import pytest
import torch

import pbe_level_ref as P
from conftest import load_golden
from evdeblurnerf_amd import weights as W
from evdeblurnerf_amd.renderer import NeRFAll
from torch_restatement import TorchVoxLevel, torch_appfeature, vox_composite

AABB = ([-1.5, -1.5, -1.0], [1.5, 1.5, 1.0])
TOL = 2e-5          # float32 golden against float64: the reference's own float32 error on these sums is ~1e-6


def _grids(sd, prefix):
    d = lambda k: torch.tensor(np.asarray(sd[prefix + k]), dtype=torch.float64)
    return [d(f"app_plane.{i}") for i in range(3)], [d(f"app_line.{i}") for i in range(3)], d("basis_mat.weight")


def _coarse(level, grids, cparams, rb, z):
    """VoxelNeRFBase.forward with composite_feature (voxnerf.py:210-239) -> per-ray colour, weights, feature map"""
    R, S = z.shape
    o, d, vd = rb[:, None, 0:3], rb[:, None, 3:6], rb[:, 8:11]
    pts = (o + d * z[..., None]).reshape(-1, 3)
    raw, geo = level(pts, vd[:, None].expand(-1, S, -1).reshape(-1, 3), torch_appfeature(*grids, pts, AABB), want_geo=True)
    _, w = vox_composite(raw.reshape(R, S, 4), z, d[:, 0])
    fmap = (w[..., None] * torch.relu(geo.reshape(R, S, -1))).sum(1)
    return P.color_rows_autograd(cparams, fmap, vd, 4), w, fmap


@pytest.mark.parametrize("pre", ["plain.", "awp."])
def test_float64_restatement_reproduces_G44(pre):
    g = load_golden("G44_pbe_train")
    gc, gf = [int(v) for v in g[pre + "grid_coarse"]], [int(v) for v in g[pre + "grid_fine"]]
    sd = W.make_train_call_state_dict(32, gc, gf)
    sub = lambda prefix: {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    lc, lf = TorchVoxLevel(sub("mlp_coarse.")), TorchVoxLevel(sub("mlp_fine."))
    gridc, gridf = _grids(sd, "mlp_coarse."), _grids(sd, "mlp_fine.")
    cparams = P.color_params(sub("mlp_coarse."))
    K = W.synthetic_camera()
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    R, Pn = g[pre + "weight"].shape
    z0 = torch.linspace(0., 1., 16, dtype=torch.float32).double().expand(R * Pn, 16)
    with torch.no_grad():
        # stage 0: coarse_render on the kernel's first set of rays
        rb0 = NeRFAll.ray_batch_train(400, 400, K, t64(g[pre + "new_rays0"]).reshape(-1, 3, 2))
        rgb0_pts, _, _ = _coarse(lc, gridc, cparams, rb0, z0)
        rgb0_pts = rgb0_pts.reshape(R, Pn, 3)
        rgb0 = (rgb0_pts * t64(g[pre + "weight0"])[..., None]).sum(1)
        # stage 1: the c2f render on the golden's merged sample positions
        rb = NeRFAll.ray_batch_train(400, 400, K, t64(g[pre + "new_rays"]).reshape(-1, 3, 2))
        rgb1_pts, _, _ = _coarse(lc, gridc, cparams, rb, z0)
        zm = t64(g[pre + "z_vals"])
        St = zm.shape[1]
        ptm = (rb[:, None, 0:3] + rb[:, None, 3:6] * zm[..., None]).reshape(-1, 3)
        ftm = torch.cat([torch_appfeature(*gridc, ptm, AABB), torch_appfeature(*gridf, ptm, AABB)], -1)
        raw = lf(ptm, rb[:, None, 8:11].expand(-1, St, -1).reshape(-1, 3), ftm).reshape(R * Pn, St, 4)
        rgb_pts, _ = vox_composite(raw, zm, rb[:, 3:6])
        w1 = t64(g[pre + "weight"])[..., None]
        rgb_pts, rgb1_pts = rgb_pts.reshape(R, Pn, 3), rgb1_pts.reshape(R, Pn, 3)
        out = dict(rgb=(rgb_pts * w1).sum(1), rgb1=(rgb0 + (rgb1_pts * w1).sum(1)) / 2, stage0_rgb_pts0=rgb0_pts[:, 0], stage1_rgb_pts0=rgb_pts[:, 0],
                   stage1_rgb1_pts0=rgb1_pts[:, 0])
    for k, v in out.items():
        err = float(np.abs(v.numpy() - g[pre + "out." + k].astype(np.float64)).max())
        assert err < TOL, (k, err)
    # the order matters: without the halving, or with the per-sample colours composited instead of the per-ray network, G44 is missed
    assert float(np.abs((out["rgb1"] * 2 - rgb0).numpy() - g[pre + "out.rgb1"]).max()) > 100 * TOL


def test_G44_holds_data_only_and_both_cases():
    g = load_golden("G44_pbe_train")
    for pre in ("awp.", "plain."):
        for k in ("new_rays0", "weight0", "new_rays", "weight", "z_vals", "tv", "loss", "out.rgb", "out.rgb1", "out.stage0_rgb_pts0"):
            assert pre + k in g, pre + k
        names = [k for k in g if k.startswith(pre + "g.mlp_") and k.endswith(".summary")]
        assert len(names) == 24, len(names)                     # 5 network + 7 grid tensors per level (no colour biases)
        assert any(k.startswith(pre + "g.kernel.") for k in g)
    assert "awp.out.rgb_awp" in g and "plain.out.rgb_awp" not in g
    assert all(v.dtype.kind in "fiu" for v in g.values())
