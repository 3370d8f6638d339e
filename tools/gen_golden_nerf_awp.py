#!/usr/bin/env python
"""Generate tests/golden/G45_nerf_awp_train.npz by RUNNING the imported reference on the CPU (build container only; needs the reference tree):

    python tools/gen_golden_nerf_awp.py

(1) NeRFAll.forward IN TRAINING MODE with mode='nerf' and kernel_use_awp (networks/renderer.py:277-378): the reference's real
RigidBlurringModel -> render of the P warped rays per pixel through two 4 x 64 NeRF networks with (6, 2) frequencies, built with
extract_feature="before_linear" (renderer.py:39) -> the real AdaptiveWeightProposal(input_ch=64) (run_nerf.py:223: input_ch = netwidth) on
the fine network's per-sample feature (renderer.py:238-257) -> the compositions.  8 pixels x P = 5, 16 + 16 samples, perturb = 0, no density
noise.  The NeRF and embedding weights are seed-derived (evdeblurnerf_amd.weights) and not stored; kernel and proposal as in golden G32
(tools/gen_golden.py _train_call_model), whose record format this file keeps: the kernel's outputs (a stub replays them on the GPU box),
every output, and torch.autograd gradients of a fixed projection of all outputs w.r.t. every NeRF parameter (norm, seeded projection,
element pins), every proposal parameter, new_rays, weight and img_embed (full).

(2) `feat.*`: the reference's NeRF.eval in float64 on case `a` of tests/nerf_generic_ref.py with extract_feature "after_linear" and
"before_linear": the two features tests/nerf_generic_ref.py GenericNerf returns as feature1 / feature2.

Data only; this file imports the reference under the stubs of tools/gen_golden.py and uses that file's helpers."""
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
P, R, SEED, N_IMGS = 5, 8, 45, 6
D, WIDTH, L, LV = 4, 64, 6, 2
OUT_KEYS = ("rgb", "rgb1", "rgb_awp", "stage1_rgb_pts0", "stage1_rgb1_pts0")


def nerf_state_dict(seed=SEED):
    """both networks, as the test rebuilds them"""
    ic, icv = W.pe_dim(L), W.pe_dim(LV)
    sd = dict(W.prefixed(W.make_nerf_state_dict(seed * 10 + 3, D, WIDTH, input_ch=ic, input_ch_views=icv), "mlp_coarse"))
    sd.update(W.prefixed(W.make_nerf_state_dict(seed * 10 + 4, D, WIDTH, input_ch=ic, input_ch_views=icv), "mlp_fine"))
    return sd


def _model():
    """GG._train_call_model with mode='nerf' networks and a proposal that reads netwidth channels"""
    import ref_import
    from networks.dpnerf.awp import AdaptiveWeightProposal
    from networks.dpnerf.blurmodel import RigidBlurringModel
    from networks.embedding import ViewEmbedding
    from networks.renderer import NeRFAll
    torch.manual_seed(SEED)
    view_embed = ViewEmbedding(num_embed=N_IMGS, embed_dim=32, init_params="normal")
    kern = RigidBlurringModel(feat_ch=0, num_motion=P - 1, D_r=1, W_r=32, D_v=1, W_v=32, D_w=1, W_w=32, output_ch_r=3, output_ch_v=3,
                              rv_window=0.1, use_origin=True, view_embed=view_embed, W=view_embed.out_channels)
    awp = AdaptiveWeightProposal(input_ch=WIDTH, num_motion=P - 1, use_origin=True, D_sam=4, W_sam=64, D_mot=1, W_mot=32, dir_freq=2,
                                 rgb_freq=2, depth_freq=3, ray_dir_freq=2, view_feature_ch=view_embed.out_channels)
    awp.load_state_dict({k: t(v) for k, v in W.make_awp_embed_state_dict(SEED * 10 + 1, input_ch=WIDTH).items()}, strict=False)
    rs = np.random.RandomState(SEED * 10 + 2)
    bn = awp.MAM.Corr.convd[1]
    with torch.no_grad():
        kern.r_linear.weight.mul_(2e4)
        kern.v_linear.weight.mul_(2e4)
        bn.weight.copy_(t(rs.uniform(0.5, 1.5, 32).astype(np.float32)))
        bn.bias.copy_(t((rs.standard_normal(32) * 0.2).astype(np.float32)))
        bn.running_mean.copy_(t((rs.standard_normal(32) * 0.1).astype(np.float32)))
        bn.running_var.copy_(t(rs.uniform(0.5, 2.0, 32).astype(np.float32)))
        for conv, k in ((awp.MAM.Corr.conva, 8.0), (awp.MAM.Corr.convb, 8.0), (awp.MAM.Corr.convc, 8.0), (awp.MAM.Corr.line_conv_att, 30.0)):
            conv.weight.mul_(k)
    args = ref_import.blurfactory_args(mode="nerf", N_importance=16, N_samples=16, kernel_use_awp=True, kernel_ptnum=P, rgb_add_bias=True,
                                       netdepth=D, netwidth=WIDTH, netdepth_fine=D, netwidth_fine=WIDTH, multires=L, multires_views=LV)
    with contextlib.redirect_stdout(io.StringIO()):
        model = NeRFAll(args, kern, awp)
    sd = nerf_state_dict()
    own = [k for k in model.state_dict() if k.startswith(("mlp_coarse.", "mlp_fine."))]
    assert set(own) == set(sd), set(own) ^ set(sd)
    model.load_state_dict({k: t(np.asarray(v).copy()) for k, v in sd.items()}, strict=False)
    assert model.extract_feature == "before_linear" and model.mlp_fine.extract_feature == "before_linear"
    return model, kern, awp


class _Replay(torch.nn.Module):
    """stands where the blur kernel stands and returns recorded outputs as autograd leaves in the run's dtype (the real kernel casts its rays
    to float32, blurmodel.py:166, so a float64 run of the call replays the float32 run's kernel outputs -- as the GPU test does)"""

    def __init__(self, kern, rec, dtype):
        super().__init__()
        self.rbk_weighted_sum = kern.rbk_weighted_sum
        self.leaf = {k: t(rec[k]).to(dtype).requires_grad_(True) for k in ("new_rays", "weight", "img_embed")}

    def forward(self, H, W_, K, rays, rays_info, feats=None, return_img_embed=False, **kw):
        return self.leaf["new_rays"], self.leaf["weight"], None, ({"img_embed": self.leaf["img_embed"]} if return_img_embed else {})


def _run(dtype, draw, replay=None):
    """one training call of the reference in `dtype` -> {name: numpy}; gradients as full arrays under 'G.<name>'.  replay: a float32
    run's record, whose kernel outputs stand in for the kernel"""
    model, kern, awp = _model()             # (built in float32 whatever the run's dtype: the modules' own initial draws are the same values)
    old_dtype, old_float = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(dtype)
    if dtype == torch.float64:              # the renderer casts its rays with .float() (renderer.py:432-441): the identity in the float64 run
        torch.Tensor.float = lambda self, *a, **k: self
    try:
        model.to(dtype)
        Dt = lambda a: t(a).to(dtype)
        model.train(True)
        rays = W.synthetic_rays(SEED + draw, R)
        rs = np.random.RandomState(4501 + 100 * draw)
        images_idx = rs.randint(0, N_IMGS, (R, 1)).astype(np.int64)
        proj = {k: rs.standard_normal((R, 3)).astype(np.float32) for k in OUT_KEYS}
        awp_before = GG._awp_sd(awp)
        if replay is not None:
            model.kernelsnet = _Replay(kern, replay, dtype)
            cap, hk = dict(model.kernelsnet.leaf), None
        else:
            cap, hk = GG._capture_kernel(kern)
        seen = {}
        hk2 = awp.register_forward_hook(lambda m, i, o: seen.update(feature=n(i[0]).copy(), z_vals=n(i[1]).copy(), rays_d=n(i[2]).copy(), awp_out=n(o).copy()))
        # the kernel's img_embed output IS its own branches' input: an identity node in front of the proposal separates the gradient that
        # arrives through the proposal (what a replayed kernel output can receive) from the total (as in G32)
        hk3 = awp.register_forward_pre_hook(lambda m, i: (seen.update(vf_awp=i[3] * 1.0), (i[0], i[1], i[2], seen["vf_awp"]))[1])
        with torch.enable_grad():
            rgb, rgb1, other_loss, other_tensors = model(400, 400, Dt(W.synthetic_camera()), chunk=1 << 20, rays=Dt(rays), rays_info={"images_idx": t(images_idx)},
                                                         force_naive=False, return_pts0_rgb=True, **GG.TRAIN_CALL_KW)
            outs = dict(rgb=rgb, rgb1=rgb1, rgb_awp=other_tensors["rgb_awp"], stage1_rgb_pts0=other_tensors["stage1_rgb_pts0"],
                        stage1_rgb1_pts0=other_tensors["stage1_rgb1_pts0"])
            loss = sum((outs[k] * Dt(proj[k])).sum() for k in proj)
            lv = [(k, p) for k, p in model.named_parameters() if k.startswith(("mlp_coarse.", "mlp_fine."))]
            ap = [("awp." + k, p) for k, p in awp.named_parameters() if not k.startswith("MAM.conv.")]
            lf = [("new_rays", cap["new_rays"]), ("weight", cap["weight"]), ("img_embed", seen["vf_awp"])]
            named = lv + ap + lf
            grads = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
        for h in (hk, hk2, hk3):
            if h is not None:
                h.remove()
        assert set(other_loss) == set() and set(other_tensors) == {"rgb_awp", "stage1_img_embed", "stage1_rgb_pts0", "stage1_rgb1_pts0"}, (set(other_loss), set(other_tensors))
        assert seen["feature"].shape == (R * P, 32, WIDTH) and all(g is not None for g in grads[:len(lv)])
        o = dict(rays=rays, images_idx=images_idx, new_rays=n(cap["new_rays"]), weight=n(cap["weight"]), img_embed=n(cap["img_embed"]),
                 loss=np.float64(loss.item()), awp_in_z_vals=seen["z_vals"], awp_in_rays_d=seen["rays_d"], awp_out=seen["awp_out"], **awp_before)
        o.update({"out." + k: n(v) for k, v in outs.items()})
        o.update({"proj." + k: v for k, v in proj.items()})
        o.update({"G." + k: n(g) for (k, _), g in zip(named, grads) if g is not None})
        bn = awp.MAM.Corr.convd[1]
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            o["awp.after." + k] = n(getattr(bn, k))
        return o
    finally:
        torch.set_default_dtype(old_dtype)
        torch.Tensor.float = old_float


Z_TOL = 5e-6
# what tests/test_gpu_train_call.py's G32_CASES asks of the float32-grade mode (all-pixel outputs, network gradients median / worst, AWP and
# kernel side), and the pixels on common samples the test asks for (G32: 6 of 32; here 2 of 8)
REF_BOUNDS = dict(out_all=3e-5, level_med=2.5e-4, level=3e-3, side=2e-2, tight=2)


def _conditioning(o32, o64):
    """from the reference alone: the share of pixels whose P rays carry the same importance samples (to Z_TOL) in float32 and float64, and
    the float32 run's error against the float64 run, measured as the tests measure"""
    sys.path.insert(0, os.path.join(GG.ROOT, "tests"))
    from torch_restatement import grad_summary
    dz = np.abs(o32["awp_in_z_vals"].astype(np.float64) - o64["awp_in_z_vals"]).max(-1).reshape(R, P).max(-1)
    err = {k: float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in o32 if k.startswith("out.")}
    lvl = []
    for i, k in enumerate(k for k in o32 if k.startswith("G.mlp_")):
        a, b = grad_summary(o32[k], 7000 + i)[0], grad_summary(o64[k], 7000 + i)[0]
        lvl.append(max(abs(a[0] - b[0]), abs(a[1] - b[1])) / b[0])
    side = [float(np.linalg.norm(o32[k].astype(np.float64) - o64[k]) / max(np.linalg.norm(o64[k]), 1e-30))
            for k in o32 if k.startswith("G.") and not k.startswith("G.mlp_") and k != "G.awp.MAM.linear.bias"]
    return float((dz < Z_TOL).mean()), err, np.array(lvl), max(side)


def train_call():
    """With perturb = 0 the resampling's u sits on cdf knots, and alpha_linear.bias' gradient is a cancelling sum over all samples: between
    a float32 and a float64 run of the REFERENCE a draw can lose its common sample positions or be 1e-2 off on that tensor.  The tests
    hold the library's float32-grade mode to G32's bounds, which only make sense where the reference's own float32 arithmetic meets them:
    rays, image ids and projections are redrawn (rays seed 45 + draw, RandomState(4501 + 100 draw)) until the reference's float32 run is
    within REF_BOUNDS of its float64 run.  Decided on the reference alone; ref_f32_err.* records the reference's own float32 error."""
    for draw in range(40):
        o32 = _run(torch.float32, draw)
        o64 = _run(torch.float64, draw, replay=o32)
        share, err, lvl, side = _conditioning(o32, o64)
        print(f"   draw {draw}: {share:.2f} of the pixels keep their samples in float32; float32 error of the reference: outputs {max(err.values()):.1e}, "
              f"NeRF gradients median {np.median(lvl):.1e} / worst {lvl.max():.1e}, AWP / kernel side {side:.1e}")
        if max(err.values()) < REF_BOUNDS["out_all"] and np.median(lvl) < REF_BOUNDS["level_med"] and lvl.max() < REF_BOUNDS["level"] \
                and side < REF_BOUNDS["side"] and share * R >= REF_BOUNDS["tight"]:
            break
    else:
        raise AssertionError("no draw on which the reference's float32 run meets REF_BOUNDS against its float64 run")
    o = {k: v for k, v in o32.items() if not k.startswith("G.")}
    GG._grad_summaries([(k[2:], v) for k, v in o32.items() if k.startswith("G.mlp_")], o, "g.")
    o.update({"g." + k[2:]: v for k, v in o32.items() if k.startswith("G.") and not k.startswith("G.mlp_")})
    o.update({"ref_f32_err." + k: np.float64(v) for k, v in err.items()})
    o["ref_f32_err.level"], o["ref_f32_err.side"], o["ref_f32_err.tight_share"] = lvl.astype(np.float64), np.float64(side), np.float64(share)
    o["draw"] = np.int64(draw)
    return o


def eval_features():
    """the reference's NeRF.eval on case `a` of tests/nerf_generic_ref.py, float64, both extract_feature settings"""
    sys.path.insert(0, os.path.join(GG.ROOT, "tests"))
    import nerf_generic_ref as G
    import ref_import
    from networks.embedding import get_embedder
    from networks.nerf import NeRF
    Dn, Wd, Ln, Lvn, skip, _, _, _ = G.CASES["a"]
    rb, z, _ = G.case_inputs("a")
    pts, dirs = G.positions(rb, z)
    x = torch.cat([get_embedder(Ln)[0](pts), get_embedder(Lvn)[0](dirs)], -1)
    out = {}
    for kind in ("after_linear", "before_linear"):
        net = NeRF(D=Dn, W=Wd, input_ch=3 * (1 + 2 * Ln), input_ch_views=3 * (1 + 2 * Lvn), output_ch=4, skips=[] if skip is None else [skip],
                   use_viewdirs=True, rgb_add_bias=True, extract_feature=kind)
        ref_import.load_np_state_dict(net, G.case_state_dict("a"))
        with torch.no_grad():
            raw, feat = net.double().eval(x)
        out["feat.raw"], out["feat." + kind] = raw.numpy(), feat.numpy()
    return out


def main():
    arrays = train_call()
    arrays.update(eval_features())
    arrays = {k: (np.asarray(v, dtype=np.float32) if np.asarray(v).dtype == np.float64 and not k.startswith("feat.") else np.asarray(v))
              for k, v in arrays.items()}
    path = os.path.join(GG.OUT, "G45_nerf_awp_train.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {os.path.relpath(path, GG.ROOT)}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
