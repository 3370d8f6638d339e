"""Pins the float64 loss-side reference of tests/test_gpu_loss.py (tests/loss_ref.py) before any kernel is held to it: to the goldens the
real reference computed (G10, G11, G12, G14, G15, G20; float32 torch results, so they are held to the same 2 u E as a kernel, on the rows
that clear the ReLU condition where a learn CRF is live), its hand-written backwards to torch float64 autograd of the plain forward (1e-12
of the terms' magnitude), and the AWP scan with eps = 1e-10 to the reference's lines restated as torch ops (the restatement that
tests/test_gpu_train.py differentiates).  CPU only; needs neither a GPU nor the oracle."""
import numpy as np
import pytest
import torch

from loss_ref import (U, awp_integrate, awp_integrate_autograd, awp_integrate_bwd, blur_loss, blur_loss_autograd, blur_loss_bwd,
                      weighted_sum)
from conftest import load_golden

K = 2.0


def within(got, ref, E, k=K):
    got, ref, E = (torch.as_tensor(np.asarray(t), dtype=torch.float64) for t in (got, ref, E))
    return bool(((got - ref).abs() <= k * U * E + 2.0 ** -120).all()), float(((got - ref).abs() / (U * E + 1e-300)).max())


def awp_inputs(rs, N, S, C, scales=(0.0, 0.05, 1.0, 8.0, 300.0)):
    feat = np.abs(rs.standard_normal((N, S, C))) * rs.choice(scales, size=(N, 1, 1))
    z = np.sort(rs.uniform(2, 6, (N, S)), -1)
    if S > 2:
        z[1::3, S // 2] = z[1::3, S // 2 - 1]
    d = rs.standard_normal((N, 3))
    d[N // 2] = 0.0                                                               # a zero direction: dist = 0, d rays_d = 0
    return feat.astype(np.float32), z.astype(np.float32), d.astype(np.float32)


def test_G10_weighted_sum():
    g = load_golden("G10_rbk_weighted_sum")
    for k in ("rgb", "depth", "acc"):
        x = g[k].reshape(24, 10, -1)
        v, E = weighted_sum(x, g["ccw"])
        ok, worst = within(g["o_" + k].reshape(24, -1), v, E)
        assert ok, (k, worst)
    for k in ("rgb0", "z_std", "weights", "depth_feature"):
        v, E = weighted_sum(g["ex_" + k].reshape(24, 10, -1), g["ccw"])
        ok, worst = within(g["o_" + k].reshape(24, -1), v, E)
        assert ok, (k, worst)


def test_G15_follows_the_form_without_the_stabiliser():
    """the golden is a float32 torch result: there `- alpha + (1. + 1e-10)` adds float32(1 + 1e-10) == 1, so it follows eps = 0 (held to
    2 u E); eps = 1e-10 moves every output by at most C 1e-10 sum_s |alpha f| (each of the <= C factors of Q grows by 1e-10, Q <= 1)"""
    g = load_golden("G15_awp_feature_integration")
    for tag in ("a", "b"):
        feat = g[f"{tag}_feat"]
        S, C = feat.shape[-2:]
        f = feat.reshape(-1, S, C)
        v0, E0 = awp_integrate(f, g[f"{tag}_z"], g[f"{tag}_rays_d"])
        ok, worst = within(g[f"{tag}_out"].reshape(-1, C), v0, E0)
        assert ok, (tag, worst)
        v1, _ = awp_integrate(f, g[f"{tag}_z"], g[f"{tag}_rays_d"], eps=1e-10)
        x = torch.tensor(f).double()
        assert ((v1 - v0).abs() <= 1.01 * C * 1e-10 * x.sum(1)).all()
        assert float((v1 - v0).abs().max()) > 0


@pytest.mark.parametrize("eps", [0.0, 1e-10])
@pytest.mark.parametrize("S,C", [(1, 5), (2, 64), (5, 1), (9, 64), (7, 20), (4, 70), (6, 130)])
def test_awp_forward_and_backward_match_float64_autograd(S, C, eps):
    """the division-free hand-written backward against autograd of awp.py:58-75 restated in float64 (the second witness of the forward,
    with and without the reference's 1e-10), incl. opaque channels, a zero rays_d row, duplicate z and S = 1"""
    rs = np.random.RandomState(S * 1000 + C)
    N = 7
    feat, z, d = awp_inputs(rs, N, S, C, scales=(0.0, 0.05, 1.0, 8.0, 40.0))
    g = rs.standard_normal((N, C))
    a = [torch.tensor(t).double().requires_grad_(True) for t in (feat, z, d)]
    out = awp_integrate_autograd(*a, eps=eps)
    v, E = awp_integrate(feat, z, d, eps=eps)
    assert ((v - out.detach()).abs() <= 1e-12 * (E + v.abs())).all()
    (out * torch.tensor(g)).sum().backward()
    r = awp_integrate_bwd(feat, z, d, g, eps=eps)
    # the restatement forms om as 1 - alpha (+ eps): 2^-53 absolute per factor of Q, where the reference's e + eps is relative
    slack = 2.0 ** -48 * C * float(np.abs(g).max()) * (1 + float(feat.max())) ** 2 * (1 + float(np.ptp(z)) * float(np.linalg.norm(d, axis=-1).max()))
    for name, ref in (("d_feat", a[0].grad), ("d_z", a[1].grad), ("d_rays_d", a[2].grad)):
        ref = torch.nan_to_num(ref) if name == "d_rays_d" else ref              # autograd's norm backward at |d| = 0
        assert ((r[name] - ref).abs() <= 1e-12 * (r["E_" + name] + ref.abs()) + slack).all(), (name, float((r[name] - ref).abs().max()))
        assert torch.isfinite(r["E_" + name]).all() and (r["E_" + name] >= 0).all()
    assert (r["d_rays_d"][N // 2] == 0).all()


def test_awp_forward_bound_holds_for_a_float32_torch_evaluation():
    """the forward evaluated by torch in float32 (the golden's form, sequential sums) stays inside 2 u E at opaque and empty rays"""
    rs = np.random.RandomState(11)
    for S, C in ((33, 64), (8, 100), (3, 256)):
        feat, z, d = awp_inputs(rs, 24, S, C)
        got = awp_integrate_autograd(torch.tensor(feat), torch.tensor(z), torch.tensor(d))
        v, E = awp_integrate(feat, z, d)
        ok, worst = within(got, v, E)
        assert ok, (S, C, worst)


def blur_inputs(rs, R, P):
    rgb_p = rs.uniform(0.02, 1, (R, P, 3)).astype(np.float32)
    rgb0_p = rs.uniform(0.02, 1, (R, P, 3)).astype(np.float32)
    lg = rs.standard_normal((2, R, P))
    w = 1 / (1 + np.exp(-lg))
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    tgt, tgt0 = rs.uniform(0, 1, (R, 3)).astype(np.float32), rs.uniform(0, 1, (R, 3)).astype(np.float32)
    return rgb_p, rgb0_p, w[0], w[1], tgt, tgt0


@pytest.mark.parametrize("map_type", ["none", "gamma"])
def test_blur_backward_matches_float64_autograd(map_type):
    rs = np.random.RandomState(5)
    for R, P in ((1, 1), (5, 3), (22, 10)):
        rgb_p, rgb0_p, w1, w2, tgt, tgt0 = blur_inputs(rs, R, P)
        g = rs.standard_normal(5)
        for has0 in (False, True):
            for has2 in (False, True):
                for hast in (False, True):
                    kw = dict(rgb0_p=rgb0_p if has0 else None, w2=w2 if has2 else None, tgt0=tgt0 if hast else None)
                    lv = {k: torch.tensor(v).double().requires_grad_(True) for k, v in (("rgb_p", rgb_p), ("rgb0_p", rgb0_p), ("w1", w1), ("w2", w2))}
                    p = blur_loss_autograd(lv["rgb_p"], lv["w1"], torch.tensor(tgt).double(), rgb0_p=lv["rgb0_p"] if has0 else None,
                                           w2=lv["w2"] if has2 else None, tgt0=torch.tensor(tgt0).double() if hast else None, map_type=map_type)
                    fwd = blur_loss(rgb_p, w1, tgt, map_type=map_type, **kw)
                    for k in range(5):
                        assert abs(float(p[k].detach()) - float(fwd["partial"][k])) <= 1e-12 * float(fwd["E_partial"][k] + 1e-300)
                    assert float(fwd["partial"][5]) == 3 * R
                    sum(gk * pk for gk, pk in zip(g, p)).backward()
                    r = blur_loss_bwd(rgb_p, w1, tgt, g, map_type=map_type, **kw)
                    names = ["rgb_p", "w1"] + (["rgb0_p"] if has0 else []) + (["w2"] if has2 else [])
                    for nme in names:
                        got, ref, E = r["d_" + nme], lv[nme].grad, r["E_d_" + nme]
                        assert ((got - ref).abs() <= 1e-12 * (E + ref.abs())).all(), (nme, has0, has2, hast)
                    assert ("d_rgb0_p" in r) == has0 and ("d_w2" in r) == has2


def _assemble(p, E, flw, w_pts0):
    c = torch.tensor([1 - flw, 1 - flw, flw, w_pts0, w_pts0], dtype=torch.float64)
    n = float(p[5])
    # golden: five float32 means, combined with ~8 float32 operations
    return float((p[:5] * c).sum() / n), float((E[:5] * c).sum() / n + 8 * (p[:5] * c).abs().sum() / n)


def test_G14_blur_loss_assembly():
    g = load_golden("G14_loss_assembly")
    for cfg in ("blender", "cdavis"):
        flw, w_pts0, _ = [float(v) for v in g[f"{cfg}_scalars"]]
        R = g[f"{cfg}_target"].shape[0]
        ccw = g[f"{cfg}_ccw"]
        o = blur_loss(g[f"{cfg}_rgb_p"].reshape(R, -1, 3), ccw[0], g[f"{cfg}_target"], rgb0_p=g[f"{cfg}_rgb0_p"].reshape(R, -1, 3), w2=ccw[1],
                      tgt0=g[f"{cfg}_target_pts0"], map_type="gamma" if cfg == "blender" else "none")
        loss, E = _assemble(o["partial"], o["E_partial"], flw, w_pts0)
        assert abs(loss - float(g[f"{cfg}_img_loss"])) <= K * U * E, (cfg, abs(loss - float(g[f"{cfg}_img_loss"])) / (U * E))
        pts0, E0 = _assemble(o["partial"], o["E_partial"], 0.0, 1.0)
        pts0 -= float(o["partial"][:2].sum() / o["partial"][5])
        assert abs(pts0 - float(g[f"{cfg}_pts0"])) <= K * U * E0, cfg


def test_G20_blur_gradients():
    """d total / d (rgb_p, rgb0_p, w1, w2) of the golden: the blur branch only reaches them; g[k] = coefficient / count"""
    g = load_golden("G20_loss_grads")
    for cfg in ("blender", "cdavis"):
        flw, w_pts0, _ = [float(v) for v in g[f"{cfg}_scalars"]]
        R = g[f"{cfg}_target"].shape[0]
        ccw = g[f"{cfg}_ccw"]
        gk = np.array([1 - flw, 1 - flw, flw, w_pts0, w_pts0]) / (3 * R)
        r = blur_loss_bwd(g[f"{cfg}_rgb_p"].reshape(R, -1, 3), ccw[0], g[f"{cfg}_target"], gk, rgb0_p=g[f"{cfg}_rgb0_p"].reshape(R, -1, 3), w2=ccw[1],
                          tgt0=g[f"{cfg}_target_pts0"], map_type="gamma" if cfg == "blender" else "none")
        for k in ("rgb_p", "rgb0_p", "w1", "w2"):
            ref, E = r["d_" + k], r["E_d_" + k] + 4 * r["d_" + k].abs()            # + the golden's own mean / weight scalings
            ok, worst = within(g[f"{cfg}_g.{k}"].reshape(ref.shape), ref, E)
            assert ok, (cfg, k, worst)


# ---- response curves and the event loss -------------------------------------------------------------------------------------------
from evdeblurnerf_amd import weights as W
from loss_ref import crf, event_loss, event_loss_autograd, event_loss_bwd, pack_params, unpack_params


def held(name, got, ref, E, safe=None, min_share=0.95):
    got, ref, E = (torch.as_tensor(np.asarray(t), dtype=torch.float64) for t in (got, ref, E))
    got = got.reshape(ref.shape)
    if safe is not None:
        assert float(safe.double().mean()) >= min_share, (name, float(safe.double().mean()))
        got, ref, E = got[safe], ref[safe], E[safe]
    ok, worst = within(got, ref, E)
    assert ok, (name, worst)


def test_G11_crf():
    g = load_golden("G11_crf")
    x, f2, f32 = g["x"].reshape(-1, 3), g["f2"], g["f32"]
    f2 = f2.reshape(-1, f2.shape[-1])
    f32 = f32.reshape(-1, 3, f32.shape[-1])
    p2 = pack_params(W.make_crf_state_dict(41, 2), 2)
    p0 = pack_params(W.make_crf_state_dict(43, 0), 0)
    held("rgb_gamma", g["rgb_gamma"], *crf(x, None, None, "gamma")[:2])
    for key, kw in (("luma_learn_f2", dict(feat=f2, luma=0)), ("luma_learn_nofeat", dict(feat=None, luma=0)), ("luma_chunked", dict(feat=None, luma=0)),
                    ("luma_learn_skip", dict(feat=f2, luma=0, skip_learn=True)), ("tone_learn_f32", dict(feat=f32, luma=-1))):
        v, E, safe = crf(x, kw.pop("feat"), p2, "learn", **kw)
        held(key, g[key], v, E, safe)
    v, E, safe = crf(x, f2, p2, "learn", luma=0)
    held("luma_learn_keep", g["luma_learn_keep"].reshape(-1, 3)[:, :1], v, E, safe)
    v, E, safe = crf(x, None, None, "none")
    assert np.array_equal(v.numpy().astype(np.float32), g["rgb_none"].reshape(-1, 3))
    held("luma_learn0", g["luma_learn0"], *crf(x, None, p0, "learn", luma=0))
    for code, key in ((0, "luma_gamma"), (1, "luma_gamma_rec709"), (2, "luma_gamma_avg")):
        held(key, g[key], *crf(x, None, None, "gamma", luma=code))


def _egm(p, E):
    return float(p[:2].sum() / p[2]), float(E[:2].sum() / p[2] + 4 * p[:2].abs().sum() / p[2])


def test_G12_egm_loss():
    """egm_loss on tone-mapped lumas: the identity curve, tonemap_only, bii entering as 1 x cum_neg (losses.egm_loss)"""
    g = load_golden("G12_egm_loss")
    bii = g["bii"].reshape(-1)
    N = bii.shape[0]
    zeros = np.zeros(N, np.float32)
    first = np.zeros((N, 3), np.uint8)
    first[:, 0] = 1
    ex = lambda a: np.ascontiguousarray(np.broadcast_to(a.reshape(N, -1), (N, 3)))
    for key, ls, le, cm, cw in (("loss_plain", ex(g["ls"]), ex(g["le"]), first, None), ("loss_mask", g["ls3"], g["le3"], g["cmask"], None),
                                ("loss_mask_w", g["ls3"], g["le3"], g["cmask"], [0.4, 0.2, 0.4])):
        r = event_loss(ls, le, bii, zeros, 1.0, 0.0, tonemap_only=True, cmask=cm, cw=cw)
        v, E = _egm(r["partial"], r["E_partial"])
        assert abs(v - float(g[key])) <= K * U * E, (key, abs(v - float(g[key])) / (U * E))


def _event_cfg(g, cfg):
    thr = 0.2 if cfg == "blender" else 0.25
    kw = dict(add_bii=1) if cfg == "blender" else dict(add_bii=2, tonemap_only=True, cmask=g[f"{cfg}_cmask"], cw=[0.4, 0.2, 0.4])
    return (g[f"{cfg}_es"], g[f"{cfg}_ee"], g[f"{cfg}_cn"], g[f"{cfg}_cp"], thr, thr), dict(start0=g[f"{cfg}_es0"], end0=g[f"{cfg}_ee0"], map_type="learn", **kw)


def test_G14_event_loss():
    g = load_golden("G14_loss_assembly")
    params = pack_params(W.make_crf_state_dict(51, 2), 2)
    for cfg in ("blender", "cdavis"):
        a, kw = _event_cfg(g, cfg)
        r = event_loss(*a, params=params, **kw)
        assert bool(r["safe"].all()), (cfg, float(r["safe"].double().mean()))      # the golden's events all clear the ReLU condition
        v, E = _egm(r["partial"], r["E_partial"])
        assert abs(v - float(g[f"{cfg}_egm"])) <= K * U * E, (cfg, abs(v - float(g[f"{cfg}_egm"])) / (U * E))


def test_G20_event_gradients():
    """d total / d (es, ee, es0, ee0) and d total / d (event-CRF parameters, weights x 3) of the golden: g_fine = g_coarse = w_egm / sum w"""
    g = load_golden("G20_loss_grads")
    csd = {k: (v * (3.0 if v.ndim == 2 else 1.0)).astype(np.float32) for k, v in W.make_crf_state_dict(51, 2).items()}
    params = pack_params(csd, 2)
    for cfg in ("blender", "cdavis"):
        a, kw = _event_cfg(g, cfg)
        w_egm = float(g[f"{cfg}_scalars"][2])
        sw = float(event_loss(*a, params=params, **kw)["partial"][2])
        r = event_loss_bwd(*a, w_egm / sw, w_egm / sw, params=params, **kw)
        safe = r["safe"]
        for k, nme in (("es", "d_start"), ("ee", "d_end"), ("es0", "d_start0"), ("ee0", "d_end0")):
            held(f"{cfg} {k}", g[f"{cfg}_g.{k}"], r[nme], r["E_" + nme] + 4 * r[nme].abs(), safe)
        if bool(safe.all()):                                          # the parameter gradient sums over every event
            gp = unpack_params(r["d_params"], "cpu")
            Ep = unpack_params(r["E_d_params"], "cpu")
            for name, key, sl in (("linear.0.weight", "w0", np.s_[:, :3]), ("linear.0.bias", "b0", np.s_[:]), ("linear.2.weight", "w1", np.s_[:]),
                                  ("linear.2.bias", "b1", np.s_[:]), ("linear.4.weight", "w2", np.s_[:]), ("linear.4.bias", "b2", np.s_[:]),
                                  ("linear.6.weight", "w3", np.s_[:]), ("linear.6.bias", "b3", np.s_[...])):
                held(f"{cfg} crf.{name}", g[f"{cfg}_g.crf.{name}"].reshape(gp[key][sl].shape), gp[key][sl], Ep[key][sl] + 4 * gp[key][sl].abs())
            assert (gp["w0"][:, 3:] == 0).all()


def draw_events(rs, n):
    """the generator of the GPU test: colours U(0.05, 0.95), counts 0..3, a one-hot colour mask"""
    ev = lambda: rs.uniform(0.05, 0.95, (n, 3)).astype(np.float32)
    cm = np.zeros((n, 3), np.uint8)
    cm[np.arange(n), rs.randint(0, 3, n)] = 1
    return ev(), ev(), ev(), ev(), -rs.randint(0, 4, n).astype(np.float32), rs.randint(0, 4, n).astype(np.float32), cm


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_relu_filter_drops_at_most_5_percent(scale):
    """the share of drawn events with a pre-activation inside 2 u of its own propagated bound (12 evaluations per event)"""
    sd = {k: (v * (scale if v.ndim == 2 else 1.0)).astype(np.float32) for k, v in W.make_crf_state_dict(51, 2).items()}
    params = pack_params(sd, 2)
    for n in (277, 4096, 65536):
        es, ee, es0, ee0, cn, cp, cm = draw_events(np.random.RandomState(n), n)
        for kw in (dict(add_bii=1), dict(add_bii=2, tonemap_only=True, cmask=cm), dict(add_bii=0)):
            safe = event_loss(es, ee, cn, cp, 0.2, 0.2, start0=es0, end0=ee0, params=params, map_type="learn", **kw)["safe"]
            share = 1 - float(safe.double().mean())
            print(f"[relu filter] weights x {scale:g} n={n} {kw.get('add_bii')}: {100 * share:.3f} % dropped")
            assert share <= 0.05


EVENT_MODES = [dict(map_type="none"), dict(map_type="gamma"), dict(map_type="learn", add_bii=1), dict(map_type="learn", add_bii=0),
               dict(map_type="learn", add_bii=2, tonemap_only=True, mask=True, cw=[0.4, 0.2, 0.4]), dict(map_type="learn", add_bii=1, skip_learn=True),
               dict(map_type="gamma", tonemap_only=True, mask=True), dict(map_type="none", tonemap_only=True), dict(map_type="learn", add_bii=1, pair=False)]


@pytest.mark.parametrize("mode", EVENT_MODES, ids=[",".join(f"{k}={v}" for k, v in m.items()) for m in EVENT_MODES])
def test_event_backward_matches_float64_autograd(mode):
    mode = dict(mode)
    rs = np.random.RandomState(9)
    n = 53
    es, ee, es0, ee0, cn, cp, cm = draw_events(rs, n)
    params = pack_params(W.make_crf_state_dict(51, 2), 2)
    pair = mode.pop("pair", True)
    cmask = cm if mode.pop("mask", False) else None
    kw = dict(mode, cmask=cmask)
    a0 = dict(start0=es0, end0=ee0) if pair else {}
    gf, gc = 0.7, -1.3
    r = event_loss_bwd(es, ee, cn, cp, 0.2, 0.25, gf, gc, params=params, **a0, **kw)
    fwd = event_loss(es, ee, cn, cp, 0.2, 0.25, params=params, **a0, **kw)
    lv = [torch.tensor(t).double().requires_grad_(True) for t in (es, ee, es0, ee0)]
    p = {k: v.clone().requires_grad_(True) for k, v in unpack_params(params, "cpu").items()}
    fine, coarse = event_loss_autograd(lv[0], lv[1], torch.tensor(cn).double(), torch.tensor(cp).double(), 0.2, 0.25, lv[2] if pair else None,
                                       lv[3] if pair else None, p, kw["map_type"], kw.get("skip_learn", False), kw.get("add_bii", 0),
                                       kw.get("tonemap_only", False), cmask, kw.get("cw"))
    assert abs(float(fine.detach()) - float(fwd["partial"][0])) <= 1e-12 * float(fwd["E_partial"][0])
    assert abs(float(coarse.detach()) - float(fwd["partial"][1])) <= 1e-12 * float(fwd["E_partial"][1]) + 0.0
    (gf * fine + gc * coarse).backward()
    names = ["d_start", "d_end"] + (["d_start0", "d_end0"] if pair else [])
    for nme, leaf in zip(names, lv):
        assert ((r[nme] - leaf.grad).abs() <= 1e-12 * (r["E_" + nme] + leaf.grad.abs())).all(), nme
    assert ("d_start0" in r) == pair
    live = kw["map_type"] == "learn" and not kw.get("skip_learn", False)
    assert ("d_params" in r) == live
    if live:
        ref = torch.cat([p[k].grad.reshape(-1) for k in ("w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")])
        assert ((r["d_params"] - ref).abs() <= 1e-12 * (r["E_d_params"] + ref.abs())).all()
        assert (unpack_params(r["d_params"], "cpu")["w0"][:, 3:] == 0).all()
