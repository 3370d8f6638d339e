"""Depth sampling on the GPU, alone: evd_sample_z (k_sample_z), evd_sample_z_pts (the same kernel writing the sample positions too, as
evd_c2f_render_rays runs it), evd_ray_batch_z (k_ray_batch_z, the fused ray packing + stratification of evd_nerf_render) and evd_points.

Exact relations (bit for bit): the fused kernel against evd_ray_batch + evd_sample_z, the positions of evd_sample_z_pts against evd_points on
its z, the lower bin edges at t_rand = 0, the end points without perturbation.  At S = 1 torch.linspace(0, 1, 1) is [0], so the one sample
is `near` (renderer.py:163-167): the far end point is asserted for S >= 2 only.

Against renderer.py:163-178 restated in float64 from the same float32 inputs, in units of u = 2^-24:
  linear    |z - ref| <= 8 u max(|near|, |far|): t carries 3 (the step, its product, the subtraction from 1), times |far - near|; 1 - t, the
            two products and the sum one each, at most max(|near|, |far|) in size
  lindisp   |1 / z - 1 / ref| <= 8 u max(1 / near, 1 / far): the two reciprocals replace near and far above (one rounding each, counted
            with the products), and the final reciprocal is one relative rounding
  perturb   12 in place of 8: the midpoint's sum, upper - lower, its product with t_rand and the sum with lower add four roundings
and z is non-decreasing along every ray.  The measured worst error / bound is printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
S_ALL = [1, 2, 3, 33, 64, 129]
R_ALL = [1, 70, 257]
RANGES = [(0.0, 1.0, 0), (2.0, 6.0, 0), (0.5, 100.0, 0), (2.0, 6.0, 1), (0.5, 100.0, 1)]          # (near, far, lindisp): lindisp only where near > 0


def make_cfg(S, near, far, lindisp, perturb, ndc):
    from evdeblurnerf_amd import _lib as L
    cfg = L.RenderCfg()
    cfg.H, cfg.W, cfg.focal, cfg.ndc, cfg.use_viewdirs, cfg.lindisp = 400, 300, 350.0, int(ndc), 1, int(lindisp)
    cfg.N_samples, cfg.N_importance, cfg.near, cfg.far, cfg.perturb = S, 0, near, far, 1.0 if perturb else 0.0
    return cfg


def run(S, R, near, far, lindisp, t_rand, ndc, seed=0):
    """every entry on the same rays -> dict of host arrays"""
    from evdeblurnerf_amd import _lib as L
    h = L.lib()
    rs = np.random.RandomState(1000 * S + R + seed)
    rays = rs.standard_normal((R, 3, 2)).astype(np.float32)
    rays[:, 2, 1] = -np.abs(rays[:, 2, 1]) - 0.1                    # d_z away from 0 (the NDC warp divides by it)
    cfg = make_cfg(S, near, far, lindisp, t_rand is not None, ndc)
    f32 = dict(dtype=torch.float32, device="cuda")
    nan = lambda *sh: torch.full(sh, float("nan"), **f32)
    d_rays = torch.tensor(rays, device="cuda")
    tr = torch.tensor(t_rand, device="cuda") if t_rand is not None else None
    st = L.stream_ptr()
    rb, z = nan(R, 11), nan(R, S)
    L.check(h.evd_ray_batch(C.byref(cfg), L.ptr(d_rays), R, L.ptr(rb), st), "evd_ray_batch")
    L.check(h.evd_sample_z(C.byref(cfg), L.ptr(rb), 11, R, L.ptr(tr), L.ptr(z), st), "evd_sample_z")
    rb_f, z_f = nan(R, 11), nan(R, S)
    L.check(h.evd_ray_batch_z(C.byref(cfg), L.ptr(d_rays), R, L.ptr(tr), L.ptr(rb_f), L.ptr(z_f), st), "evd_ray_batch_z")
    z_p, pts_p, pts = nan(R, S), nan(R, S, 3), nan(R, S, 3)
    L.check(h.evd_sample_z_pts(C.byref(cfg), L.ptr(rb), 11, R, L.ptr(tr), L.ptr(z_p), L.ptr(pts_p), st), "evd_sample_z_pts")
    L.check(h.evd_points(L.ptr(rb), 11, L.ptr(z_p), R, S, L.ptr(pts), st), "evd_points")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(rb=rb, z=z, rb_f=rb_f, z_f=z_f, z_p=z_p, pts_p=pts_p, pts=pts).items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def z_reference(S, R, near, far, lindisp, t_rand):
    """renderer.py:163-178 in float64 from the float32 near, far and t_rand"""
    near, far = float(np.float32(near)), float(np.float32(far))
    t = np.arange(S, dtype=np.float64) / (S - 1) if S > 1 else np.zeros(1)
    z = 1.0 / (1.0 / near * (1.0 - t) + 1.0 / far * t) if lindisp else near * (1.0 - t) + far * t
    z = np.broadcast_to(z, (R, S)).copy()
    if t_rand is not None:
        mids = 0.5 * (z[:, 1:] + z[:, :-1])
        upper, lower = np.concatenate([mids, z[:, -1:]], -1), np.concatenate([z[:, :1], mids], -1)
        z = lower + (upper - lower) * t_rand.astype(np.float64)
    return z


def error_ratio(z, ref, near, far, lindisp, n):
    if lindisp:
        return float(np.max(np.abs(1.0 / z.astype(np.float64) - 1.0 / ref)) / (n * U * max(1.0 / near, 1.0 / far)))
    return float(np.max(np.abs(z.astype(np.float64) - ref)) / (n * U * max(abs(near), abs(far))))


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("near,far,lindisp", RANGES)
@pytest.mark.parametrize("S", S_ALL)
def test_sample_z_entries_agree_and_match_the_float64_reference(S, near, far, lindisp, perturb):
    worst = 0.0
    for R in R_ALL:
        t_rand = None
        if perturb:
            t_rand = np.minimum(np.random.RandomState(S + R).uniform(0, 1, (R, S)).astype(np.float32), np.float32(1 - U))
        for ndc in (0, 1):
            o = run(S, R, near, far, lindisp, t_rand, ndc)
            tag = f"R={R} ndc={ndc}"
            assert not np.isnan(o["z"]).any() and not np.isnan(o["rb"]).any() and not np.isnan(o["pts"]).any(), tag
            assert np.array_equal(bits(o["z_f"]), bits(o["z"])), f"{tag}: z of evd_ray_batch_z != evd_ray_batch + evd_sample_z"
            assert np.array_equal(bits(o["rb_f"]), bits(o["rb"])), f"{tag}: packed rows of evd_ray_batch_z != evd_ray_batch"
            assert np.array_equal(bits(o["z_p"]), bits(o["z"])), f"{tag}: z of evd_sample_z_pts != evd_sample_z"
            assert np.array_equal(bits(o["pts_p"]), bits(o["pts"])), f"{tag}: pts of evd_sample_z_pts != evd_points on its z"
            assert np.array_equal(o["rb"][:, 6], np.full(R, near, np.float32)) and np.array_equal(o["rb"][:, 7], np.full(R, far, np.float32))
        z = o["z"]
        if not perturb:
            assert np.array_equal(z[:, 0], np.full(R, near, np.float32)), f"R={R}: z[:, 0] != near"
            if S >= 2:
                assert np.array_equal(z[:, -1], np.full(R, far, np.float32)), f"R={R}: z[:, -1] != far"
        assert bool((np.diff(z, axis=-1) >= 0).all()), f"R={R}: z decreases along a ray"
        r = error_ratio(z, z_reference(S, R, near, far, lindisp, t_rand), near, far, lindisp, 12 if perturb else 8)
        assert r <= 1.0, f"R={R}: error {r:.3g} x the bound"
        worst = max(worst, r)
    print(f"sample_z S={S} [{near:g}, {far:g}] lindisp={lindisp} perturb={perturb}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("near,far,lindisp", RANGES)
@pytest.mark.parametrize("S", S_ALL)
def test_zero_draw_gives_the_lower_bin_edges(S, near, far, lindisp):
    for R in R_ALL:
        off = run(S, R, near, far, lindisp, None, 0)["z"]
        on = run(S, R, near, far, lindisp, np.zeros((R, S), np.float32), 0)
        mids = (np.float32(0.5) * (off[:, 1:] + off[:, :-1])).astype(np.float32)          # float32, as the reference forms them
        lower = np.concatenate([off[:, :1], mids], -1)
        assert np.array_equal(bits(on["z"]), bits(lower)), f"R={R}"
        assert np.array_equal(bits(on["z_f"]), bits(lower)), f"R={R} (evd_ray_batch_z)"


def test_invalid_arguments_are_errors():
    from evdeblurnerf_amd import _lib as L
    h = L.lib()
    R, S = 4, 8
    rb, z, pts = torch.zeros((R, 11), device="cuda"), torch.zeros((R, S), device="cuda"), torch.zeros((R, S, 3), device="cuda")
    rays = torch.ones((R, 3, 2), device="cuda")
    st = L.stream_ptr()
    on, off = make_cfg(S, 0.0, 1.0, 0, True, 0), make_cfg(S, 0.0, 1.0, 0, False, 0)
    assert h.evd_sample_z(C.byref(on), L.ptr(rb), 11, R, None, L.ptr(z), st) != 0                      # perturb without the draw
    assert h.evd_ray_batch_z(C.byref(on), L.ptr(rays), R, None, L.ptr(rb), L.ptr(z), st) != 0
    assert h.evd_sample_z_pts(C.byref(off), L.ptr(rb), 11, R, None, L.ptr(z), None, st) != 0            # no pts
    assert h.evd_sample_z_pts(C.byref(off), L.ptr(rb), 5, R, None, L.ptr(z), L.ptr(pts), st) != 0       # no direction columns
    assert h.evd_sample_z(C.byref(off), None, 11, R, None, L.ptr(z), st) != 0                          # no packed rays
    assert h.evd_sample_z(C.byref(off), L.ptr(rb), 7, R, None, L.ptr(z), st) != 0                       # no near / far columns
    assert h.evd_ray_batch_z(C.byref(off), None, R, None, L.ptr(rb), L.ptr(z), st) != 0
    assert h.evd_ray_batch_z(C.byref(off), L.ptr(rays), R, None, None, L.ptr(z), st) != 0
    assert h.evd_ray_batch_z(C.byref(make_cfg(0, 0.0, 1.0, 0, False, 0)), L.ptr(rays), R, None, L.ptr(rb), L.ptr(z), st) != 0
    assert h.evd_sample_z_pts(C.byref(off), L.ptr(rb), 11, R, None, L.ptr(z), L.ptr(pts), st) == 0
    torch.cuda.synchronize()
