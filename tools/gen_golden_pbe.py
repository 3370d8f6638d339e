#!/usr/bin/env python
"""Generate tests/golden/G44_pbe_train.npz by RUNNING the imported reference on the CPU (build container only; needs the reference tree):

    python tools/gen_golden_pbe.py

NeRFAll.forward IN TRAINING MODE with kernel_type='PBE' (networks/renderer.py:286-378): the reference's real BlurModel (pdrf/blurmodel.py,
kernel_type PBE, the module and state dict of golden G39's `pbe` case) runs twice -- stage 0 without features, whose rays go through
coarse_render (the composite_feature coarse level: voxnerf.py:223-239), stage 1 with that render's composited features -- then the c2f
render of the stage-1 rays, the composition with the kernel's weights, rgb1 = (rgb0 + rgb1) / 2, TV x 5.  G32's small shape: 32 pixels x
P = 5, 16 + 16 samples, grids 24^3 / 48^3, perturb = 0, no density noise; level parameters from evdeblurnerf_amd.weights (seed 32).  Two
cases: `awp.` with the real AdaptiveWeightProposal of G32 (its non-RBK sums, renderer.py:331-336) and `plain.` without.

Recorded per case (data only): the kernel's outputs of both stages, the merged sample positions, rgb, rgb1, every other_tensors key, TV,
and torch.autograd gradients of sum_k <out_k, proj_k> + 0.1 TV w.r.t. every level / grid parameter (norm, seeded projection, head, element
pins -- G32's format), every kernel parameter and, with AWP, every AWP parameter (full).  This file imports the reference under the stubs of
tools/gen_golden.py and uses that file's helpers; no reference source is copied.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as GG  # noqa: E402  (installs the reference import stubs)

import torch  # noqa: E402

from evdeblurnerf_amd import weights as W  # noqa: E402

t, n = GG.t, GG.n
P, R, SEED = 5, 32, 32
OUT_KEYS = ("rgb", "rgb1", "stage0_rgb_pts0", "stage1_rgb_pts0", "stage1_rgb1_pts0")


def _kernel():
    """the BlurModel of G39's `pbe` case with its recorded state dict -> (module, that case's inputs)"""
    case = GG.SPARSE_BLUR_CASES["pbe"]
    cfg = dict(GG.SPARSE_BLUR_DEFAULTS, **{k: v for k, v in case.items() if k not in ("R", "seed", "poses_buffer")})
    g = np.load(os.path.join(GG.OUT, "G39_sparse_blur.npz"))
    sd = {k[len("pbe.sd."):]: g[k] for k in g.files if k.startswith("pbe.sd.")}
    assert cfg["num_pt"] == P
    return GG._sparse_blur_module(cfg, sd, torch.float32), {k: g["pbe." + k] for k in ("ids", "rays_x", "rays_y", "noise")}


def _model(use_awp):
    from networks.renderer import NeRFAll
    import ref_import
    kern, kin = _kernel()
    awp = GG._train_call_model(P)[2] if use_awp else None          # G32's AdaptiveWeightProposal, values and all (view features: 32 channels)
    args = ref_import.blurfactory_args(mode="c2f", N_importance=16, N_samples=16, kernel_type="PBE", kernel_use_awp=use_awp, kernel_ptnum=P,
                                       rgb_add_bias=False, **GG.PDRF_SMALL)
    with contextlib.redirect_stdout(io.StringIO()):
        model = NeRFAll(args, kern, awp)
    gc, gf = [int(v) for v in model.mlp_coarse.gridSize], [int(v) for v in model.mlp_fine.gridSize]
    sd = W.make_train_call_state_dict(SEED, gc, gf)
    for k in model.state_dict():
        if k.startswith(("mlp_coarse.", "mlp_fine.")) and k not in sd:
            raise KeyError(k)
    model.load_state_dict({k: t(np.asarray(v).copy()) for k, v in sd.items()}, strict=False)
    assert model.mlp_coarse.composite_feature and not model.mlp_fine.composite_feature
    return model, kern, awp, kin, gc, gf


def _inputs(attempt):
    """what the call reads besides the parameters: per-ray poses, the two randn_like draws of the kernel (in call order), the projections"""
    kin = _kernel()[1]
    rs = np.random.RandomState(4401 + 100 * attempt)
    poses = np.concatenate([np.eye(3, dtype=np.float32)[None].repeat(R, 0) + 0.02 * rs.standard_normal((R, 3, 3)).astype(np.float32),
                            0.1 * rs.standard_normal((R, 3, 1)).astype(np.float32)], -1)
    noise = [kin["noise"][:R].astype(np.float32), rs.standard_normal((R, P, 2)).astype(np.float32)]
    proj = {k: rs.standard_normal((R, 3)).astype(np.float32) for k in OUT_KEYS + ("rgb_awp",)}
    return dict(poses=poses, noise=noise, proj=proj, ids=kin["ids"][:R].reshape(R, 1).astype(np.int64), rays_x=kin["rays_x"][:R], rays_y=kin["rays_y"][:R])


def _run(use_awp, dtype, inp):
    """one training call of the reference in `dtype` throughout -> {name: numpy}, gradients as full arrays under 'G.<name>'"""
    old_dtype = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model, kern, awp, _, gc, gf = _model(use_awp)
        model.to(dtype)
        D = lambda a: t(a).to(dtype)
        model.train(True)
        keys = OUT_KEYS + (("rgb_awp",) if use_awp else ())
        info = {"images_idx": t(inp["ids"]), "rays_x": D(inp["rays_x"]), "rays_y": D(inp["rays_y"]), "poses": D(inp["poses"])}
        calls, seen, draws = [], {}, []
        hk = kern.register_forward_hook(lambda m, i, o: calls.append(dict(new_rays=o[0], weight=o[1], extras=o[3])))
        render = model.render
        model.render = lambda *a, **k: (lambda r: (seen.update(z_vals=n(r[3]["z_vals"]).copy()), r)[1])(render(*a, **k))
        old = torch.randn_like
        torch.randn_like = lambda x, *a, **k: (draws.append(1), D(inp["noise"][len(draws) - 1]).reshape(x.shape))[1]
        try:
            with torch.enable_grad():
                rgb, rgb1, other_loss, other_tensors = model(400, 400, D(W.synthetic_camera()), chunk=1 << 20, rays=torch.zeros((R, 3, 2), dtype=dtype),
                                                             rays_info=info, force_naive=False, return_pts0_rgb=True, **GG.TRAIN_CALL_KW)
                outs = dict(rgb=rgb, rgb1=rgb1, **{k: other_tensors[k] for k in keys if k not in ("rgb", "rgb1")})
                tv = other_loss["TV"]
                loss = sum((outs[k] * D(inp["proj"][k])).sum() for k in keys) + 0.1 * tv.sum()
                lv = [(k, p) for k, p in model.named_parameters() if k.startswith(("mlp_coarse.", "mlp_fine."))]
                kp = [("kernel." + k, p) for k, p in kern.named_parameters()]
                ap = [("awp." + k, p) for k, p in awp.named_parameters() if not k.startswith("MAM.conv.")] if use_awp else []
                lf = [("new_rays0", calls[0]["new_rays"]), ("weight0", calls[0]["weight"]), ("new_rays", calls[1]["new_rays"]), ("weight", calls[1]["weight"])]
                named = lv + kp + ap + lf
                grads = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
        finally:
            torch.randn_like = old
            hk.remove()
        assert len(draws) == 2 and len(calls) == 2, (len(draws), len(calls))
        assert set(other_loss) == {"TV"}, set(other_loss)                   # (kernel_type PBE returns no align loss)
        exp = {"stage0_rgb_pts0", "stage1_rgb_pts0", "stage1_rgb1_pts0"} | ({"rgb_awp", "stage1_img_embed"} if use_awp else set())
        assert set(other_tensors) == exp, set(other_tensors) ^ exp
        assert all(g is not None for (k, _), g in zip(named, grads) if k.startswith("mlp_")), [k for (k, _), g in zip(named, grads) if g is None]
        o = dict(new_rays0=n(calls[0]["new_rays"]), weight0=n(calls[0]["weight"]), new_rays=n(calls[1]["new_rays"]), weight=n(calls[1]["weight"]),
                 z_vals=seen["z_vals"], tv=np.float64(tv.sum().item()), loss=np.float64(loss.item()), grid_coarse=np.array(gc), grid_fine=np.array(gf))
        o.update({"out." + k: n(v) for k, v in outs.items()})
        o.update({"G." + k: n(g) for (k, _), g in zip(named, grads) if g is not None})
        if use_awp:
            o["img_embed"] = n(other_tensors["stage1_img_embed"])
            o.update(GG._awp_sd(awp))
        return o
    finally:
        torch.set_default_dtype(old_dtype)


Z_TOL = 5e-6


def _conditioning(o32, o64):
    """from the reference alone: the share of pixels whose P rays carry the same importance samples (to Z_TOL) in float32 and float64, and
    the float32 run's error against the float64 run (outputs: max abs; level gradients: (norm, projection) error / norm, as the tests measure)"""
    sys.path.insert(0, os.path.join(GG.ROOT, "tests"))
    from torch_restatement import grad_summary
    dz = np.abs(o32["z_vals"].astype(np.float64) - o64["z_vals"]).max(-1).reshape(R, P).max(-1)
    err = {k: float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in o32 if k.startswith("out.")}
    lvl = []
    for i, k in enumerate(k for k in o32 if k.startswith("G.mlp_")):
        a, b = grad_summary(o32[k], 7000 + i)[0], grad_summary(o64[k], 7000 + i)[0]
        lvl.append(max(abs(a[0] - b[0]), abs(a[1] - b[1])) / b[0])
    return float((dz < Z_TOL).mean()), err, np.array(lvl)


# what tests/test_gpu_train_call.py's G32_CASES asks of the float32-grade mode: all-pixel outputs, level gradients median / worst, pixels on common samples
REF_BOUNDS = dict(out_all=3e-5, level_med=2.5e-4, level=3e-3, tight=6)


def _case(use_awp, out, pre, attempt, select=False):
    inp = _inputs(attempt)
    o32, o64 = _run(use_awp, torch.float32, inp), _run(use_awp, torch.float64, inp)
    share, err, lvl = _conditioning(o32, o64)
    print(f"   {pre[:-1]} (draw {attempt}): {share:.2f} of the pixels keep their samples in float32; float32 error of the reference: outputs "
          f"{max(err.values()):.1e}, level gradients median {np.median(lvl):.1e} / worst {lvl.max():.1e}")
    if select and not (max(err.values()) < REF_BOUNDS["out_all"] and np.median(lvl) < REF_BOUNDS["level_med"] and lvl.max() < REF_BOUNDS["level"]
                       and share * R >= REF_BOUNDS["tight"]):
        return False
    o = {k: v for k, v in o32.items() if not k.startswith("G.")}
    GG._grad_summaries([(k[2:], v) for k, v in o32.items() if k.startswith("G.mlp_")], o, "g.")
    o.update({"g." + k[2:]: v for k, v in o32.items() if k.startswith("G.") and not k.startswith("G.mlp_")})
    o.update(poses=inp["poses"], noise0=inp["noise"][0], noise1=inp["noise"][1])
    o.update({"proj." + k: v for k, v in inp["proj"].items() if use_awp or k != "rgb_awp"})
    o.update({"ref_f32_err." + k: np.float64(v) for k, v in err.items()})
    o["ref_f32_err.level"] = lvl.astype(np.float64)
    o["ref_f32_err.tight_share"] = np.float64(share)
    out.update({pre + k: v for k, v in o.items()})
    out.update(ids=inp["ids"], rays_x=inp["rays_x"], rays_y=inp["rays_y"], draw=np.int64(attempt))
    return True


def G44_pbe_train():
    """With perturb = 0 the resampling's u sits on cdf knots: between a float32 and a float64 run of the REFERENCE only 0.03 .. 0.28 of the pixels
    keep their importance samples (to 5e-6), and the float32 run's level gradients are up to 1e-3 (median) from the float64 run's.  The tests hold
    this library's float32-grade mode to G32's bounds, which only make sense where the reference's own float32 arithmetic meets them: the kernel's
    per-ray poses and second noise draw are redrawn (seed 4401 + 100 draw) until, without AWP, the reference's float32 run is within REF_BOUNDS of
    its float64 run.  Decided on the reference alone; both cases use that draw, and ref_f32_err.* records the reference's own float32 error."""
    out = {}
    for draw in range(40):
        if _case(False, out, "plain.", draw, select=True):
            break
    else:
        raise AssertionError("no draw on which the reference's float32 run meets REF_BOUNDS against its float64 run")
    _case(True, out, "awp.", draw)
    path = os.path.join(GG.OUT, "G44_pbe_train.npz")
    np.savez_compressed(path, **{k: (np.asarray(v, dtype=np.float32) if np.asarray(v).dtype == np.float64 and np.asarray(v).ndim > 1 else np.asarray(v))
                                 for k, v in out.items()})
    print(f"  wrote {os.path.relpath(path, GG.ROOT)}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    G44_pbe_train()
