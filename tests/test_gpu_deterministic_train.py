"""The deterministic training mode end to end: the fixed-order loss reductions (evd_crf_set_deterministic) and whole training iterations
with NeRFAll.enable_training(..., deterministic=True) repeat bit for bit, and agree with the default (float-atomic) path within the
tolerances the existing tests hold that path to.

Loss entries: the deterministic forms go through the cases of tests/test_gpu_loss.py (its float64 reference, its bounds K u E) with the
switch on, at R = 257 pixels x P = 5 and N = 1000 events -- no multiple of a workgroup, more than one workgroup.
Whole iteration: the G32 model and the G33 loop of tests/test_gpu_train_call.py, two iterations, run twice from the same state."""
import numpy as np
import pytest
import torch
from types import SimpleNamespace

import test_gpu_loss as TL
import test_gpu_train_call as TC
from conftest import load_golden
from evdeblurnerf_amd import _lib as L, weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class deterministic:
    """the switch on a CRF of test_gpu_loss.py's cache, off again afterwards (the cache is shared with that module's tests)"""

    def __init__(self, *crfs):
        self.crfs = crfs

    def __enter__(self):
        for c in self.crfs:
            c.set_deterministic(True)

    def __exit__(self, *exc):
        for c in self.crfs:
            c.set_deterministic(False)


# ---- loss entries ------------------------------------------------------------------------------------------------------------------
R, P, N = 257, 5, 1000
EV_MODE = "learn-add_bii1"            # a live learn CRF with the pos-neg features


def test_blur_loss_deterministic_forms_match_float64():
    """the bounds of test_gpu_loss.py::test_blur_loss_matches_float64, every presence combination of (rgb0_p, w2, target_pts0)"""
    crf = TL.crf_of("gamma")
    with deterministic(crf):
        for i, pres in enumerate(TL.PRESENCE):
            TL.blur_case(f"det k_blur_loss_det gamma R{R} P{P} {pres}", "gamma", False, R, P, pres, 900 + i, partial0=i % 2 == 1, dev_entry=i % 2 == 0)


def test_event_loss_deterministic_forms_match_float64():
    crf, _ = TL.learn_crf(51, 2, 1.0)
    with deterministic(crf):
        for pair in (True, False):
            TL.event_case(f"det k_event_loss_det {EV_MODE} N{N} pair{int(pair)}", TL.EVENT_MODES[EV_MODE], N, pair, dev_entry=pair, want_params=True, seed=950 + pair)


def test_blur_loss_deterministic_repeats_and_accumulates():
    crf = TL.crf_of("gamma")
    rgb_p, rgb0_p, w1, w2, tgt, tgt0 = TL.blur_inputs(R, P, 31, False)
    g = [float(np.float32(v)) for v in (0.7, -1.3, 0.45, 2.1, -0.6)]
    with deterministic(crf):
        runs = []
        for _ in range(3):
            partial = torch.zeros(8, device=DEV)
            TL.blur_fwd(crf, False, rgb_p, rgb0_p, w1, w2, tgt, tgt0, partial, False)
            o = TL.blur_bwd(crf, False, rgb_p, rgb0_p, w1, w2, tgt, tgt0, g, True)
            runs.append([partial, o["d_rgb_p"], o["d_rgb0_p"], o["d_w1"], o["d_w2"]])
        for r in runs[1:]:
            assert all(same_bits(a, b) for a, b in zip(runs[0], r))
        assert float(runs[0][0][:5].abs().min()) > 0 and float(runs[0][0][5]) == 3 * R
        twice = torch.zeros(8, device=DEV)                                  # "accumulates into partial": ONE partial[k] += sum per call
        TL.blur_fwd(crf, False, rgb_p, rgb0_p, w1, w2, tgt, tgt0, twice, False)
        TL.blur_fwd(crf, False, rgb_p, rgb0_p, w1, w2, tgt, tgt0, twice, False)
        assert same_bits(twice, runs[0][0] + runs[0][0])


def test_event_loss_deterministic_repeats_and_accumulates():
    crf, _ = TL.learn_crf(51, 2, 1.0)
    es, ee, es0, ee0, cn, cp, cm = TL.event_draw(N, 41)
    with deterministic(crf):
        runs = []
        for _ in range(3):
            partial = torch.zeros(4, device=DEV)
            TL.event_call("evd_event_loss_reduce", crf, False, 1, False, es, ee, es0, ee0, cn, cp, None, None, (L.ptr(partial),))
            o = [torch.full_like(es, float("nan")) for _ in range(4)] + [torch.full((TL.LR.CRF_NPARAM,), float("nan"), device=DEV)]
            TL.event_call("evd_event_loss_bwd", crf, False, 1, False, es, ee, es0, ee0, cn, cp, None, None, (0.7, -1.3) + tuple(L.ptr(t) for t in o))
            runs.append([partial] + o)
        for r in runs[1:]:
            assert all(same_bits(a, b) for a, b in zip(runs[0], r))
        assert float(runs[0][0][2]) == N and float(runs[0][5].abs().max()) > 0 and all(bool(torch.isfinite(t).all()) for t in runs[0])
        twice = torch.zeros(4, device=DEV)
        for _ in range(2):
            TL.event_call("evd_event_loss_reduce", crf, False, 1, False, es, ee, es0, ee0, cn, cp, None, None, (L.ptr(twice),))
        assert same_bits(twice, runs[0][0] + runs[0][0])


# ---- whole iterations --------------------------------------------------------------------------------------------------------------
def _model(seed, g, prec, awp_kind, kernel, grads_in_place, deterministic):
    """test_gpu_train_call.py's _model with the AWP optional (awp_kind 'none') and the deterministic switch"""
    from evdeblurnerf_amd.awp import FusedAWP
    from evdeblurnerf_amd.renderer import NeRFAll
    gc, gf = [int(v) for v in g["grid_coarse"]], [int(v) for v in g["grid_fine"]]
    sd = W.make_train_call_state_dict(seed, gc, gf)
    Pk = g["s0.weight"].shape[1]
    args = SimpleNamespace(mode="c2f", multires=10, multires_views=4, use_viewdirs=True, N_importance=16, kernel_type="RBK", kernel_use_awp=awp_kind != "none",
                           rgb_activate="sigmoid", sigma_activate="relu", bounding_box=TC.AABB, coarse_num_layers=2, coarse_num_layers_color=3,
                           coarse_hidden_dim=64, coarse_hidden_dim_color=64, coarse_app_dim=32, coarse_app_n_comp=[64, 16, 16], coarse_n_voxels=24 ** 3,
                           kernel_feat_cnl=15, fine_num_layers=2, fine_num_layers_color=3, fine_hidden_dim=256, fine_hidden_dim_color=256,
                           fine_geo_feat_dim=128, fine_app_dim=32, fine_app_n_comp=[64, 16, 16], fine_n_voxels=48 ** 3)
    awp = awpnet = None
    if awp_kind != "none":
        awp = TC._awp_module(seed, g, Pk)
        awpnet = FusedAWP(awp, precision="f16") if awp_kind == "fused" else awp
    model = NeRFAll(args, sd, kernelsnet=kernel, awpnet=awpnet, precision=prec)
    kw = dict(deterministic=True) if deterministic else {}
    return model.enable_training(sd, grads_in_place=grads_in_place, **kw).train(), awp


def run_iterations(prec, awp_kind, in_place, det, steps):
    """the loop of test_G33_five_iterations_follow_the_reference_trajectory with the library's Adam; returns the losses (device scalars),
    the gradients after the first backward and the parameters after the last step"""
    from evdeblurnerf_amd import optim as O
    from evdeblurnerf_amd.losses import blur_loss_partials_autograd, event_loss_from_partials, event_loss_partials_autograd
    from evdeblurnerf_amd.tonemapping import CRF
    g = load_golden("G33_train_trajectory")
    lrate, lrate_decay, flw, w_pts0, w_egm, w_tv, thr = (float(v) for v in g["scalars"])
    kern = TC.ReplayKernel(g, prefix="s{}.")
    model, awp = _model(33, g, prec, awp_kind, kern, in_place, det)
    csd = W.make_crf_state_dict(331, extra_features=2)
    csd = {k: (v * np.float32(3.0) if np.asarray(v).ndim == 2 else v) for k, v in csd.items()}
    crf_rgb, crf_ev = CRF("gamma"), CRF("learn", state_dict=csd, extra_features=2)
    if det:
        crf_rgb.set_deterministic(True)
        crf_ev.set_deterministic(True)
    crf_flat = crf_ev.flat_params("cuda")
    groups = [{"params": model.grad_vars, "lr": lrate}, {"params": model.grad_vars_vol, "lr": lrate}, {"params": [crf_flat], "lr": lrate}]
    for gr in groups:
        gr.setdefault("initial_lr", gr["lr"])
    opt = O.Adam(groups, lr=lrate, betas=(0.9, 0.999), model=model, zero_grads=in_place)
    K = W.synthetic_camera()
    T = lambda k: torch.tensor(g[k], device=DEV)
    rays, ev_start, ev_end, target, target_pts0, cn, cp = (T(k) for k in ("rays", "ev_start", "ev_end", "target", "target_pts0", "cn", "cp"))
    info = {"images_idx": T("images_idx")}
    ones = torch.ones((rays.shape[0], 1), device=DEV)
    losses, grads, side = [], None, None
    for i in range(steps):
        kern.step = i
        rgb, rgb0, other, tens = model(400, 400, K, 1 << 20, rays=rays, rays_info=info, force_naive=False, return_pts0_rgb=True, **TC.CALL_KW)
        pa = blur_loss_partials_autograd(crf_rgb, rgb[:, None], ones, target, rgb0_p=rgb0[:, None])
        pc = blur_loss_partials_autograd(crf_rgb, tens["stage1_rgb_pts0"][:, None], ones, target_pts0, rgb0_p=tens["stage1_rgb1_pts0"][:, None])
        n = pa.detach()[5]
        loss = (pa[0] + pa[1]) / n * (1 - flw) + (pc[0] + pc[1]) / n * w_pts0
        if awp_kind != "none":
            pb = blur_loss_partials_autograd(crf_rgb, tens["rgb_awp"][:, None], ones, target)
            loss = loss + pb[0] / n * flw
        loss = loss + other["TV"].mean() * w_tv
        s, s0, _, _ = model(400, 400, K, 1 << 20, rays=ev_start, rays_info=None, force_naive=True, **TC.CALL_KW)
        e, e0, _, _ = model(400, 400, K, 1 << 20, rays=ev_end, rays_info=None, force_naive=True, **TC.CALL_KW)
        pe = event_loss_partials_autograd(crf_ev, crf_flat, s, e, cn, cp, thr, thr, start0=s0, end0=e0, add_bii="pos-neg")
        loss = loss + event_loss_from_partials(pe) * w_egm
        if not in_place:
            opt.zero_grad()
        loss.backward()
        if i == 0:
            grads = {k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}
            grads["crf"] = crf_flat.grad.detach().clone()
            side = {k: kern.last[k].grad.detach().clone() for k in ("new_rays", "weight", "img_embed") if kern.last[k].grad is not None}
        opt.step()
        crf_ev.load_params(crf_flat)
        for gr in opt.param_groups:
            gr["lr"] = gr["initial_lr"] * (0.1 ** ((i + 1) / (lrate_decay * 1000)))           # run_nerf.py:603-613
        losses.append(loss.detach().clone())
    params = {k: v.detach().clone() for k, v in model.named_parameters()}
    params["crf"] = crf_flat.detach().clone()
    torch.cuda.synchronize()
    return losses, grads, side, params


def test_enable_training_takes_the_deterministic_switch():
    g = load_golden("G33_train_trajectory")
    model, _ = _model(33, g, "f16", "none", TC.ReplayKernel(g, prefix="s{}."), False, True)
    assert model._deterministic and all(lv.net._deterministic for lv in model._levels if lv is not None)
    model, _ = _model(33, g, "f16", "none", TC.ReplayKernel(g, prefix="s{}."), False, False)
    assert not model._deterministic and not any(lv.net._deterministic for lv in model._levels if lv is not None)


DEFAULT_RUN = {}


def default_grads(prec, awp_kind):
    """one backward of the default (float-atomic) path: shared by the two grads_in_place settings of a case"""
    if (prec, awp_kind) not in DEFAULT_RUN:
        DEFAULT_RUN[(prec, awp_kind)] = run_iterations(prec, awp_kind, False, False, 1)
    return DEFAULT_RUN[(prec, awp_kind)]


# (precision, AWP): the tolerances of G32_CASES for the agreement with the default path.  AWP 'none' has no case of its own in G32_CASES:
# its level gradients are held to the f16x3 numbers (the AWP branch adds gradient, it does not change the levels' arithmetic)
CASES = {("f16", "fused"): TC.G32_CASES[("f16", "fused")], ("f16x3", "none"): TC.G32_CASES[("f16x3", "torch")]}


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("prec,awp_kind", list(CASES))
def test_two_iterations_repeat_bit_for_bit(prec, awp_kind, in_place):
    tol = CASES[(prec, awp_kind)]
    a = run_iterations(prec, awp_kind, in_place, True, 2)
    b = run_iterations(prec, awp_kind, in_place, True, 2)
    assert all(bool(torch.isfinite(l)) for l in a[0])
    diff = []
    for name, x, y in (("loss", dict(enumerate(a[0])), dict(enumerate(b[0]))), ("grad", a[1], b[1]), ("side", a[2], b[2]), ("param", a[3], b[3])):
        assert set(x) == set(y)
        diff += [f"{name} {k}" for k in x if not same_bits(x[k], y[k])]
    assert not diff, f"{len(diff)} tensors differ between two runs from the same state: {diff[:12]}"
    # ... and it is the same gradient as the default path's, within G32's per-mode tolerances
    _, dg, dside, _ = default_grads(prec, awp_kind)
    assert set(dg) == set(a[1])
    lv = {k: TC.rel(a[1][k].cpu().numpy(), dg[k].cpu().numpy()) for k in dg if k.startswith(("mlp_coarse.", "mlp_fine."))}
    sd = {k: TC.rel(a[1][k].cpu().numpy(), dg[k].cpu().numpy()) for k in dg if k not in lv and float(dg[k].abs().max()) > 0
          and "MAM.linear.bias" not in k}                 # (that bias: analytically zero gradient, rounding noise on both sides)
    sd.update({k: TC.rel(a[2][k].cpu().numpy(), dside[k].cpu().numpy()) for k in dside})
    top = lambda d: {k: f"{v:.1e}" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:5]}
    print(f"det vs default [{prec}, {awp_kind} AWP, in_place={in_place}] level gradients: median {np.median(list(lv.values())):.1e} worst {top(lv)}; side {top(sd)}")
    assert np.median(list(lv.values())) < tol["level_med"] and max(lv.values()) < tol["level"], top(lv)
    assert max(sd.values()) < tol["side"], top(sd)
