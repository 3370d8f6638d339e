"""The per-sample feature of a mode='nerf' network under training (evd_nerf_mlp_train_feature / evd_nerf_mlp_backward_feature: the generic
float32-grade kernels with the feature as a plane of the store and its gradient as one more addend of the backward) against the float64
restatement tests/nerf_generic_ref.py GenericNerf, whose out["feature1"] / out["feature2"] are the reference's two extract_feature settings
(pinned to the reference's NeRF class by golden G45, tests/test_nerf_feature_ref.py).

Cases: a, c, f of nerf_generic_ref.CASES and s, the standard 8 x 256 / (10, 4) / skips [4] network, which reaches the generic kernels only
through these entries.  d feature = RandomState(10).normal * gscale / sqrt(W); d raw and d feature are zero on the samples that carry a
ReLU tie (a float64 pre-activation within TAU = 2e-6 of zero), at most 10 % of a case.  Bounds: forward 2e-5, parameter gradients 5e-6
relative L2, gradients that reach the rays 2e-4 -- those of tests/test_gpu_nerf_generic_train.py."""
import functools

import numpy as np
import pytest
import torch

import nerf_generic_ref as G
from evdeblurnerf_amd import weights as W
from test_gpu_train import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name: (D, W, L, Lv, skip or None, R, S, scale of d raw), as nerf_generic_ref.CASES
S_CASE = (8, 256, 10, 4, 4, 33, 7, 1e-2)
NAMES = ["a", "c", "f", "s"]
GENERIC = ["a", "c", "f"]       # networks that the plain training entries run on the generic kernels too
KINDS = {1: "after_linear", 2: "before_linear"}


def case(name):
    return S_CASE if name == "s" else G.CASES[name]


@functools.lru_cache(maxsize=None)
def case_state_dict(name):
    if name != "s":
        return G.case_state_dict(name)
    D, Wd, L, Lv, skip, _, _, _ = S_CASE
    return W.make_nerf_state_dict(400 + ord("s"), D, Wd, input_ch=W.pe_dim(L), input_ch_views=W.pe_dim(Lv), skips=(skip,))


def case_inputs(name):
    """ray batch [R, 11], z [R, S], d raw [R, S, 4], d feature [R, S, W], float32; the tie samples are not zeroed yet"""
    _, Wd, _, _, _, R, S, gscale = case(name)
    rb, z = G.make_inputs(R, S, 6)
    rs = np.random.RandomState(9)
    d_raw = (rs.normal(size=(R, S, 4)) * gscale * np.exp(rs.uniform(-4, 0, (R, S, 1)))).astype(np.float32)      # nerf_generic_ref.case_inputs
    d_feat = (np.random.RandomState(10).normal(size=(R, S, Wd)) * gscale / np.sqrt(Wd)).astype(np.float32)
    return rb, z, d_raw, d_feat


def ref_net(name):
    D, Wd, L, Lv, skip, _, _, _ = case(name)
    return G.GenericNerf(case_state_dict(name), D, Wd, L, Lv, skip)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """float64, computed once and shared: dict with raw [n, 4], feature [n, W], d_raw / d_feat (float32, tie samples zeroed), frac (fraction
    of samples zeroed), grads {state-dict key: gradient of sum(raw d_raw) + sum(feature d_feat)} and rays [R, 11] (the same loss's
    gradient with respect to the ray batch, through the float32 sample positions as in test_gpu_nerf_generic_train.py)"""
    rb, z, d_raw, d_feat = case_inputs(name)
    R, S = z.shape
    net = ref_net(name)
    rb64 = torch.tensor(rb, dtype=torch.float64, requires_grad=True)
    z64 = torch.tensor(z, dtype=torch.float64)
    pts32 = torch.tensor(rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None], dtype=torch.float64)
    expr = rb64[:, None, 0:3] + rb64[:, None, 3:6] * z64[..., None]
    pts = (pts32 + (expr - expr.detach())).reshape(-1, 3)
    dirs = rb64[:, None, 8:11].expand(-1, S, -1).reshape(-1, 3)
    pre, out = {}, {}
    raw = net(pts, dirs, pre, out=out)
    feat = out[f"feature{kind}"]
    ties = G.tie_samples(pre).numpy()
    d_raw, d_feat = d_raw.copy(), d_feat.copy()
    d_raw.reshape(-1, 4)[ties] = 0.0
    d_feat.reshape(-1, d_feat.shape[-1])[ties] = 0.0
    loss = (raw * torch.tensor(d_raw, dtype=torch.float64).reshape(-1, 4)).sum() + \
        (feat * torch.tensor(d_feat, dtype=torch.float64).reshape(feat.shape)).sum()
    loss.backward()
    grads = {k: net.p[k.replace(".", "_")].grad.clone() for k in case_state_dict(name)}
    return dict(raw=raw.detach(), feature=feat.detach(), d_raw=d_raw, d_feat=d_feat, frac=float(ties.mean()), grads=grads, rays=rb64.grad.clone())


def make_net(name, kind=1, prec="f16x3"):
    from evdeblurnerf_amd.nerf import NeRF
    D, Wd, L, Lv, skip, _, _, _ = case(name)
    return NeRF(case_state_dict(name), D=D, W=Wd, multires=L, multires_views=Lv, skips=() if skip is None else (skip,), precision=prec,
                extract_feature=KINDS[kind])


def T(x):
    return torch.tensor(x, device=DEV)


@pytest.mark.parametrize("name", NAMES)
def test_raw_is_the_plain_training_forward_bit_for_bit(name):
    """raw of the forward with the feature against NeRF.mlpforward_train without it, bit for bit.  Cases a, c, f: both calls run the generic
    kernel on one stream.  Case s: the plain call is the pipelined split-float16 kernel, which adds the skip layer's k-steps in the order
    [h_0 .. h_13 | pe | h_14, h_15]; the feature forward reads a stream of its own in that order (evd_nerf::stream_pd) and gives the same bits
    (on the generic stream's order [pe | h]: 269 of 924 values one unit in the last place off, 1.19e-07)."""
    net = make_net(name)
    rb, z = case_inputs(name)[:2]
    raw = net.mlpforward_train(T(rb), T(z), want_feature=True)[0]
    plain = net.mlpforward_train(T(rb), T(z))[0]
    print(f"[case {name}] max |raw with the feature - raw without| = {(raw - plain).abs().max().item():.2e}; "
          f"{int((raw != plain).sum())} of {raw.numel()} values differ")
    assert torch.equal(raw, plain)


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_forward(name, kind):
    """the feature is a view of the store; it is the inference kernel's, bit for bit, where that kernel is the generic one; raw and feature
    within 2e-5 of float64"""
    net = make_net(name, kind)
    rb, z = case_inputs(name)[:2]
    ref = reference(name, kind)
    raw, store, feat = net.mlpforward_train(T(rb), T(z), want_feature=True)
    assert feat.shape == (z.shape[0], z.shape[1], net.W) and feat.dtype == torch.float32
    assert feat.data_ptr() >= store.data_ptr() and feat.data_ptr() + feat.numel() * 4 <= store.data_ptr() + store.numel()    # a view, not a copy
    if name in GENERIC:
        assert torch.equal(raw, net.mlpforward(T(rb), T(z), precision="f16x3")[0])
        assert torch.equal(feat, net.mlpforward(T(rb), T(z), want_feature=True, precision="f16x3")[1])
    e_raw = (raw.reshape(-1, 4).cpu().double() - ref["raw"]).abs().max().item()
    e_feat = (feat.reshape(-1, net.W).cpu().double() - ref["feature"]).abs().max().item()
    print(f"[case {name}, {KINDS[kind]}] max |raw - float64| = {e_raw:.2e}, max |feature - float64| = {e_feat:.2e} "
          f"(max |feature| = {ref['feature'].abs().max().item():.2f})")
    assert e_raw < 2e-5
    assert e_feat < 2e-5


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_match_float64_autograd(name, kind):
    """NeRF.mlp_train(want_feature=True) as one autograd node: parameter gradients of sum(raw d_raw) + sum(feature d_feature) within 5e-6
    relative L2 per block, the gradients that reach the rays within 2e-4"""
    net = make_net(name, kind)
    rb_np, z_np = case_inputs(name)[:2]
    ref = reference(name, kind)
    assert ref["frac"] <= G.TIE_CAP
    flat = net.flat_params(case_state_dict(name))
    rb = torch.tensor(rb_np, device=DEV, requires_grad=True)
    raw, feat = net.mlp_train(flat, rb, T(z_np), want_feature=True)
    ((raw * T(ref["d_raw"])).sum() + (feat * T(ref["d_feat"])).sum()).backward()
    got = net.unflatten(flat.grad)
    assert set(got) == set(ref["grads"])
    errs = {k: rel_l2(g.cpu().double(), ref["grads"][k]) for k, g in got.items()}
    worst = max(errs, key=errs.get)
    gr = rb.grad.cpu().double()
    rays = {"rays_o": rel_l2(gr[:, 0:3], ref["rays"][:, 0:3]), "rays_d": rel_l2(gr[:, 3:6], ref["rays"][:, 3:6]),
            "viewdirs": rel_l2(gr[:, 8:11], ref["rays"][:, 8:11])}
    print(f"[case {name}, {KINDS[kind]}] worst parameter gradient vs float64 autograd: {worst} {errs[worst]:.2e} ({100 * ref['frac']:.1f} % of the "
          "samples zeroed as ties); ray gradients:", {k: f"{v:.1e}" for k, v in rays.items()})
    assert errs[worst] < 5e-6, {k: f"{v:.1e}" for k, v in errs.items()}
    assert max(rays.values()) < 2e-4, rays


def _backward(net, name, kind, d_feat, accumulate_into=None):
    rb, z = case_inputs(name)[:2]
    ref = reference(name, kind)
    raw, store, feat = net.mlpforward_train(T(rb), T(z), want_feature=True)
    return net.mlp_backward_flat(T(ref["d_raw"]), store, d_feature=d_feat, feature_store=True, want_rays=True, accumulate_into=accumulate_into)


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", GENERIC)
def test_without_a_feature_gradient_is_the_plain_backward(name, kind):
    net = make_net(name, kind)
    rb, z = case_inputs(name)[:2]
    ref = reference(name, kind)
    got = _backward(net, name, kind, None)
    raw, store = net.mlpforward_train(T(rb), T(z))
    pts = (T(rb)[:, None, 0:3] + T(rb)[:, None, 3:6] * T(z)[..., None]).contiguous()
    want = net.mlp_backward_flat(T(ref["d_raw"]), store, pts=pts, ray_batch=T(rb))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert got[0].abs().max().item() > 0


@pytest.mark.parametrize("name", GENERIC)
def test_node_without_a_feature_gradient_is_the_plain_node(name):
    """NeRF.mlp_train(want_feature=True) with a gradient for raw alone (the node's d_feature is None) against NeRF.mlp_train without the
    feature under the same d raw: the parameter gradient and the gradient that reaches the rays, bit for bit"""
    net = make_net(name)
    rb_np, z_np, d_raw = case_inputs(name)[:3]
    grads = []
    for want in (True, False):
        flat = net.flat_params(case_state_dict(name))
        rb = torch.tensor(rb_np, device=DEV, requires_grad=True)
        out = net.mlp_train(flat, rb, T(z_np), want_feature=want)
        raw = out[0] if want else out
        (raw * T(d_raw)).sum().backward()
        grads.append((flat.grad, rb.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][0].abs().max().item() > 0 and grads[0][1].abs().max().item() > 0


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", ["a", "s"])
def test_backward_repeats_bit_for_bit_and_accumulates(name, kind):
    net = make_net(name, kind)
    d_feat = T(reference(name, kind)["d_feat"])
    first, second = _backward(net, name, kind, d_feat), _backward(net, name, kind, d_feat)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    flat = first[0]
    assert flat.abs().max().item() > 0 and bool(torch.isfinite(flat).all())
    plain = _backward(net, name, kind, None)[0]
    assert not torch.equal(plain, flat)                                     # the feature's gradient did enter
    known = torch.randn(flat.shape, generator=torch.Generator().manual_seed(3)).to(DEV) * flat.abs().mean()
    buf = known.clone()
    out = _backward(net, name, kind, d_feat, accumulate_into=buf)
    assert out[0] is None and torch.equal(out[1], first[1]) and torch.equal(out[2], first[2])
    assert torch.equal(buf, known + flat)


def test_refusals():
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.nerf import NeRF
    rb, z = case_inputs("a")[:2]
    for name in ("a", "s"):
        net = make_net(name)
        assert int(L.lib().evd_nerf_train_feature_store_bytes(net.handle, L.PREC["f16x3"], 64)) > 0
        for prec in ("f32", "f16", "bf16", "f16c", "f16m"):
            assert int(L.lib().evd_nerf_train_feature_store_bytes(net.handle, L.PREC[prec], 64)) == 0
            assert int(L.lib().evd_nerf_backward_feature_workspace_bytes(net.handle, L.PREC[prec])) == 0
            with pytest.raises(L.EvdError):
                net.mlpforward_train(T(rb), T(z), precision=prec, want_feature=True)
            raw, store, feat = net.mlpforward_train(T(rb), T(z), want_feature=True)
            with pytest.raises(L.EvdError):
                net.mlp_backward_flat(torch.zeros_like(raw), store, precision=prec, d_feature=torch.zeros_like(feat), feature_store=True)
    nv = NeRF(W.make_nerf_state_dict(31, 4, 64, use_viewdirs=False), D=4, W=64, use_viewdirs=False, precision="f16x3", extract_feature="before_linear")
    with pytest.raises(L.EvdError):
        nv.mlpforward_train(T(rb[:, :8]), T(z), want_feature=True)
    assert int(L.lib().evd_nerf_train_feature_store_bytes(nv.handle, L.PREC["f16x3"], 64)) == 0
    off, ld = L.C.c_long(0), L.C.c_long(0)
    store = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)
    raw = torch.empty((z.shape[0], z.shape[1], 4), device=DEV)
    rc = L.lib().evd_nerf_mlp_train_feature(nv.handle, L.PREC["f16x3"], L.ptr(T(rb[:, :8]).contiguous()), L.ptr(T(z)), z.shape[0], z.shape[1], L.ptr(raw), 2,
                                            L.ptr(store), store.numel(), L.C.byref(off), L.C.byref(ld), L.stream_ptr())
    assert rc == -1 and b"use_viewdirs=False" in L.lib().evd_last_error()
