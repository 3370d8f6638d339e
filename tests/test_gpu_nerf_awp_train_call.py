"""The WHOLE training call with mode='nerf' and kernel_use_awp against the reference: golden G45 (tools/gen_golden_nerf_awp.py: NeRFAll.forward
in training mode, networks/renderer.py:277-378, with the reference's real RigidBlurringModel and AdaptiveWeightProposal(input_ch=64) on the
fine NeRF network's before_linear feature, renderer.py:238-257).  4 x 64 networks with (6, 2) frequencies, 16 + 16 samples, 8 pixels x
P = 5, perturb = 0, no density noise.  As in tests/test_gpu_train_call.py a stub kernel replays the recorded outputs of the real one, and
the gradients the kernel would receive are read off them; everything behind it is this repository's path: ray packing, both networks on
the generic float32-grade kernels (the fine one with its feature output and the feature's gradient), resampling, the proposal (its sample
embedding on float32 rows of 64 channels), the compositions, backward.

Bounds: G32_CASES of tests/test_gpu_train_call.py for f16x3, the torch AWP module's row for the plain stand-in and the fused row for
FusedAWP; conftest.train_call_errors separates the pixels whose P rays carry the golden's sample positions.  The golden's draw (rays, image
ids, projections) is chosen on the reference alone, as for G44: alpha_linear.bias' gradient is a cancelling sum over all samples, and on
draws 0 and 1 the reference's own float32 run is 1.6e-2 / 3.8e-2 from its float64 run on that tensor; tools/gen_golden_nerf_awp.py redraws
until the reference's float32 run meets G32's float32-grade bounds against its float64 run (draw 2: outputs 7.4e-08, NeRF gradients median
2.2e-07, worst 5.8e-05, AWP / kernel side 1.1e-02; recorded as `ref_f32_err.*`).  On the parent commit every test here ends in
NotImplementedError or EvdError."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, maxabs, train_call_errors
from evdeblurnerf_amd import weights as W

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

DEV = "cuda"
SEED, D, WIDTH, L, LV, P = 45, 4, 64, 6, 2, 5


def nerf_state_dict():
    """tools/gen_golden_nerf_awp.py nerf_state_dict: the weights are seed-derived, the golden does not store them"""
    ic, icv = W.pe_dim(L), W.pe_dim(LV)
    sd = dict(W.prefixed(W.make_nerf_state_dict(SEED * 10 + 3, D, WIDTH, input_ch=ic, input_ch_views=icv), "mlp_coarse"))
    sd.update(W.prefixed(W.make_nerf_state_dict(SEED * 10 + 4, D, WIDTH, input_ch=ic, input_ch_views=icv), "mlp_fine"))
    return sd


def awp_module(g):
    from awp_standin import RefLikeAWP
    awp = RefLikeAWP(P=P, view_ch=g["img_embed"].shape[1], mam="corr", input_ch=WIDTH)
    sd = {k[len("awp.sd."):]: torch.tensor(g[k]) for k in g if k.startswith("awp.sd.")}
    sd.update({k: torch.tensor(v) for k, v in W.make_awp_embed_state_dict(SEED * 10 + 1, input_ch=WIDTH).items()})
    missing, unexpected = awp.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return awp.cuda().train()


def build(g, awp_kind, prec="f16x3", grads_in_place=False, kernel_type="RBK", N_importance=16):
    from evdeblurnerf_amd.awp import FusedAWP
    from evdeblurnerf_amd.renderer import NeRFAll
    from test_gpu_train_call import ReplayKernel
    sd = nerf_state_dict()
    args = SimpleNamespace(mode="nerf", netdepth=D, netwidth=WIDTH, netdepth_fine=D, netwidth_fine=WIDTH, multires=L, multires_views=LV, use_viewdirs=True,
                           rgb_activate="sigmoid", sigma_activate="relu", N_importance=N_importance, kernel_type=kernel_type, kernel_use_awp=True)
    awp = awp_module(g)
    awpnet = FusedAWP(awp) if awp_kind == "fused" else awp
    kern = ReplayKernel(g)
    model = NeRFAll(args, sd, kernelsnet=kern, awpnet=awpnet, precision=prec).enable_training(sd, grads_in_place=grads_in_place).train()
    assert model.use_awp and (model.mlp_fine or model.mlp_coarse).extract_feature == "before_linear"
    return model, kern, awp


def call(model, g, seen=None):
    from test_gpu_train_call import CALL_KW
    R = g["weight"].shape[0]
    if seen is not None:
        inner, orig = model.awpnet, model.awpnet.forward
        inner.forward = lambda df, z, rd, vf: (seen.update(z_vals=z.detach().reshape(R * P, -1).cpu().numpy(), rays_d=rd.detach().reshape(R * P, 3).cpu().numpy(),
                                                            feature=df), orig(df, z, rd, vf))[1]
    rays = torch.tensor(g["rays"], device=DEV)
    info = {"images_idx": torch.tensor(g["images_idx"], device=DEV)}
    rgb, rgb1, other_loss, other_tensors = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, rays_info=info, force_naive=False, return_pts0_rgb=True,
                                                 **CALL_KW)
    out = dict(rgb=rgb, rgb1=rgb1, rgb_awp=other_tensors["rgb_awp"], stage1_rgb_pts0=other_tensors["stage1_rgb_pts0"],
               stage1_rgb1_pts0=other_tensors["stage1_rgb1_pts0"])
    return out, other_loss, other_tensors


def projected(out, g):
    return sum((out[k] * torch.tensor(g["proj." + k], device=DEV)).sum() for k in out)


@pytest.mark.parametrize("awp_kind", ["torch", "fused"])
def test_G45_training_call_matches_the_reference(awp_kind):
    from test_gpu_train_call import G32_CASES, rel
    from torch_restatement import check_grad_elements, grad_summary
    tol = G32_CASES[("f16x3", awp_kind)]
    g = load_golden("G45_nerf_awp_train")
    model, kern, awp = build(g, awp_kind)
    if awp_kind == "fused":
        assert model.awpnet.embed.generic and model.awpnet.embed.input_ch == WIDTH
    R = g["weight"].shape[0]
    seen = {}
    out, other_loss, other_tensors = call(model, g, seen)
    assert set(other_loss) == set() and set(other_tensors) == {"rgb_awp", "stage1_img_embed", "stage1_rgb_pts0", "stage1_rgb1_pts0"}
    assert tuple(seen["feature"].shape) == (R * P, 32, WIDTH)                        # the fine network's feature on the merged samples
    assert maxabs(seen["rays_d"], g["awp_in_rays_d"]) < 2e-6
    tight, e_t, e_a = train_call_errors({k: v.detach().cpu().numpy() for k, v in out.items()}, seen["z_vals"], g, z_tol=5e-6)
    print(f"G45 [f16x3, {awp_kind} AWP] outputs: {int(tight.sum())} of {R} pixels on the golden's sample positions;", {k: f"{v:.1e}" for k, v in e_t.items()},
          "all pixels:", {k: f"{v:.1e}" for k, v in e_a.items()})
    loss = projected(out, g)
    loss.backward()
    got = {k: v.grad for k, v in model.named_parameters() if k.startswith(("mlp_coarse.", "mlp_fine."))}
    keys = [k[2:-8] for k in g if k.startswith("g.mlp_") and k.endswith(".summary")]
    assert set(keys) == set(got) == set(nerf_state_dict()), set(keys) ^ set(got)
    worst, elem = {}, {}
    for idx, key in enumerate(keys):
        a = got[key].detach().cpu().numpy()
        sm, _ = grad_summary(a, 7000 + idx)
        ref = g[f"g.{key}.summary"]
        worst[key] = max(abs(sm[0] - ref[0]), abs(sm[1] - ref[1])) / float(ref[0])
        elem[key], _ = check_grad_elements(a, g[f"g.{key}.elem_idx"], g[f"g.{key}.elem_val"], 1.0)
    top = lambda d: {k: f"{v:.1e}" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:5]}
    print(f"G45 [f16x3, {awp_kind} AWP] NeRF gradients (fine and coarse), (norm / projection error) / norm: median {np.median(list(worst.values())):.1e}, worst", top(worst))
    print(f"G45 [f16x3, {awp_kind} AWP] NeRF gradients, worst pinned element / largest:", top(elem))
    side = {}
    for k, p in awp.named_parameters():
        if "g.awp." + k not in g:
            continue
        ref = g["g.awp." + k]
        if k == "MAM.linear.bias":                   # analytically zero (the training-mode BatchNorm removes a constant added to every curve)
            assert p.grad is None or p.grad.abs().max().item() < 1e-4
            continue
        assert p.grad is not None, k
        side["awp." + k] = rel(p.grad.cpu().numpy().reshape(ref.shape), ref)
    assert any(k.startswith("awp.sample_feature_embed_layer.") for k in side)
    for k in ("new_rays", "weight", "img_embed"):
        side[k] = rel(kern.last[k].grad.cpu().numpy(), g["g." + k])
    print(f"G45 [f16x3, {awp_kind} AWP] AWP / kernel-side gradients, error / norm:", top(side))
    assert tight.sum() >= 2                                                           # (G32 asks 6 of its 32 pixels)
    assert max(v for k, v in e_t.items() if k != "rgb_awp") < tol["out"] and e_t["rgb_awp"] < tol["awp_out"], e_t
    assert max(e_a.values()) < tol["out_all"], e_a
    assert abs(loss.item() - float(g["loss"])) < 200 * tol["out_all"]
    assert np.median(list(worst.values())) < tol["level_med"] and max(worst.values()) < tol["level"], top(worst)
    assert max(side.values()) < tol["side"], top(side)


def test_fused_and_plain_proposal_agree():
    """FusedAWP (the embedding on float32 rows, the rest on the library's kernels) against the plain stand-in module on the same call"""
    from test_gpu_train_call import G32_CASES, rel
    tol = G32_CASES[("f16x3", "fused")]
    g = load_golden("G45_nerf_awp_train")
    res = {}
    for kind in ("torch", "fused"):
        model, kern, awp = build(g, kind)
        out, _, _ = call(model, g)
        projected(out, g).backward()
        res[kind] = ({k: v.detach() for k, v in out.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if k.startswith("mlp_")},
                     {k: kern.last[k].grad.clone() for k in ("new_rays", "weight", "img_embed")})
    e_out = max((res["torch"][0][k] - res["fused"][0][k]).abs().max().item() for k in res["torch"][0])
    e_lv = {k: rel(res["fused"][1][k].cpu().numpy(), res["torch"][1][k].cpu().numpy()) for k in res["torch"][1]}
    e_side = {k: rel(res["fused"][2][k].cpu().numpy(), res["torch"][2][k].cpu().numpy()) for k in res["torch"][2]}
    print(f"fused vs plain proposal: outputs {e_out:.1e}, NeRF gradients worst {max(e_lv.values()):.1e}, kernel side {max(e_side.values()):.1e}")
    assert e_out < tol["awp_out"] and max(e_lv.values()) < tol["level"] and max(e_side.values()) < tol["side"]


def test_grads_in_place_agrees():
    g = load_golden("G45_nerf_awp_train")
    grads = {}
    for in_place in (False, True):
        model, kern, awp = build(g, "torch", grads_in_place=in_place)
        out, _, _ = call(model, g)
        projected(out, g).backward()
        grads[in_place] = {k: p.grad.clone() for k, p in model.named_parameters() if k.startswith("mlp_")}
    assert len(grads[True]) == len(nerf_state_dict())
    for k, v in grads[False].items():
        assert v.abs().max().item() > 0 and torch.equal(v, grads[True][k]), k


def test_coarse_only_model_hands_the_coarse_feature():
    """N_importance = 0: the last pass is the coarse one (renderer.py:219-221), its network's feature goes to the proposal"""
    g = load_golden("G45_nerf_awp_train")
    model, kern, awp = build(g, "fused", N_importance=0)
    from test_gpu_train_call import CALL_KW
    R = g["weight"].shape[0]
    seen = {}
    inner, orig = model.awpnet, model.awpnet.forward
    inner.forward = lambda df, z, rd, vf: (seen.update(feature=df), orig(df, z, rd, vf))[1]
    rgb, rgb1, _, ot = model(400, 400, W.synthetic_camera(), 1 << 20, rays=torch.tensor(g["rays"], device=DEV),
                             rays_info={"images_idx": torch.tensor(g["images_idx"], device=DEV)}, force_naive=False, **dict(CALL_KW, N_importance=0))
    assert rgb1 is None and tuple(seen["feature"].shape) == (R * P, 16, WIDTH)
    (rgb.sum() + ot["rgb_awp"].sum()).backward()
    for k, p in model.named_parameters():
        if k.startswith("mlp_coarse."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0, k


def test_refusals():
    """before any launch: another training precision; kernel_type PBE with mode='nerf'"""
    g = load_golden("G45_nerf_awp_train")
    for prec in ("f16", "bf16"):
        model, _, _ = build(g, "torch")
        model.train_precision = prec
        with pytest.raises(NotImplementedError, match="f16x3"):
            call(model, g)
    model, _, _ = build(g, "torch")
    rb = model.ray_batch_train(400, 400, W.synthetic_camera(), torch.tensor(g["rays"], device=DEV))
    model.train_precision = "f16"
    with pytest.raises(NotImplementedError, match="f16x3"):
        model.render_rays_train(rb, None, None, 16, 16, want_feature=True)
    model, _, _ = build(g, "torch", kernel_type="PBE")
    with pytest.raises(NotImplementedError, match="mode='nerf'"):
        call(model, g)
