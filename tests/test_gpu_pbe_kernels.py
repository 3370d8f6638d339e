"""The two per-ray training steps of a composite_feature level (kernel_type PBE) through ctypes against the float64 references of
tests/pbe_level_ref.py, element by element: |kernel - ref| <= K u E with u = 2^-24, E the reference's first-order bound, K = 2 for the
second-order terms, and an absolute 2^-120 for float32 underflow.  Nothing measured on a kernel enters a bound.

  evd_raw2outputs_feat_bwd          d_sigma (inside d_raw, whose other channels must be zero), d_rows, d_rays_d (columns past 2 untouched)
  evd_voxel_color_rows_train        colour; bit-equal to evd_voxel_forward's colour for the same composited map
  evd_voxel_color_rows_backward     d_map, d_viewdirs, the six parameter gradients (NULL bias pointers, accumulate), two bit-equal runs

The colour network's ReLUs: a ray with a pre-activation inside its own error bound (pbe_level_ref `unsure`, at most 2 % of a case, decided
on the float64 forward alone) is left out -- colour and d_map rows not compared, its g_color zero so that it adds nothing to either side's
weight-gradient sums.

Measured on one MI355X, the worst error / bound over all cases, by output (the module prints this line at the end of every run):
  d_sigma 0.087, d_rows 0.25, d_rays_d 0.020; color 0.0088, d_map 0.0036, d_dirs 0.0021; d_w0 0.44, d_w1 0.41, d_w2 0.098, d_b0 0.096,
  d_b1 0.24, d_b2 0.21.  The per-ray outputs use under 1 % of their bounds (a worst-case count of roundings against random signs); the
  weight-gradient sums sit higher because their bound counts the reduction tree (rays per workgroup + workgroups) once, not per layer.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pbe_level_ref as P
import voxel_level_ref as V
from evdeblurnerf_amd import _lib as L

pytestmark = pytest.mark.gpu

U, K, TINY = 2.0 ** -24, 2.0, 2.0 ** -120
DEV = "cuda"
SHARES = {}


def check(name, got, ref, E, rows=None):
    got, ref, E = got.detach().double(), ref.double().to(got.device), E.double().to(got.device)
    if rows is not None:
        got, ref, E = got[rows], ref[rows], E[rows]
    assert torch.isfinite(got).all(), f"{name}: non-finite"
    err, bound = (got - ref).abs(), K * U * E + TINY
    share = float((err / bound).max()) if err.numel() else 0.0
    SHARES[name.split(" ")[-1]] = max(SHARES.get(name.split(" ")[-1], 0.0), share)
    print(f"{name}: worst error / bound = {share:.3g}")
    assert share <= 1.0, f"{name}: {int((err > bound).sum())} elements over {K} u E, worst share {share:.3g}"


def dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV).contiguous()


# ---- evd_raw2outputs_feat_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.FEAT_CASES, ids=[c["id"] for c in P.FEAT_CASES])
def test_feature_composite_backward_matches_float64(c):
    a = P.feat_inputs(c)
    R, S, G, st = c["R"], c["S"], c["G"], c["stride"]
    raw, rows, z, rays, noise = dev(a["raw"]), dev(a["rows"]), dev(a["z"]), dev(a["rays"]), dev(a["noise"])
    g = [dev(v) for v in a["g"]]
    d_raw, d_rows = torch.full((R, S, 4), float("nan"), device=DEV), torch.full((R, S, G), float("nan"), device=DEV)
    d_rd = torch.full((R, st), 1234.5, device=DEV)
    rd_ptr = C.c_void_p(rays.data_ptr() + 4 * a["col"])
    L.check(L.lib().evd_raw2outputs_feat_bwd(L.ptr(raw), 4, 0, L.ptr(rows), G, L.ACT[c["act"]], L.ptr(z), rd_ptr, st, L.ptr(noise), L.ACT["relu"], 0.0, R, S,
                                             L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(g[3]), L.ptr(d_raw), L.ptr(d_rows), L.ptr(d_rd), st,
                                             L.stream_ptr()), "evd_raw2outputs_feat_bwd")
    torch.cuda.synchronize()
    r = P.feat_reference(c, DEV)
    assert (d_raw[..., 1:] == 0).all(), "d_raw: a channel other than sigma is not zero"
    check(f"{c['id']} d_sigma", d_raw[..., 0], r["d_sigma"], r["E_d_sigma"])
    check(f"{c['id']} d_rows", d_rows, r["d_rows"], r["E_d_rows"])
    check(f"{c['id']} d_rays_d", d_rd[:, :3], r["d_rays_d"], r["E_d_rays_d"])
    assert (d_rd[:, 3:] == 1234.5).all(), "d_rays_d written past column 2"
    if S == 1:
        assert not d_raw.any()


def test_feature_composite_backward_layouts_and_refusals():
    """sigma in another channel of a wider raw, no d_rays_d; G and S out of range are refused"""
    c = P.FEAT_CASES[2]
    a = P.feat_inputs(c)
    R, S, G = c["R"], c["S"], c["G"]
    raw6 = torch.randn((R, S, 6), device=DEV)
    raw6[..., 4] = dev(a["raw"])[..., 0]
    rows, z, rays = dev(a["rows"]), dev(a["z"]), dev(a["rays"])
    g = [dev(v) for v in a["g"]]
    d_raw, d_rows = torch.full((R, S, 6), float("nan"), device=DEV), torch.full((R, S, G), float("nan"), device=DEV)
    call = lambda G_, S_: L.lib().evd_raw2outputs_feat_bwd(L.ptr(raw6), 6, 4, L.ptr(rows), G_, L.ACT[c["act"]], L.ptr(z), L.ptr(rays), 3, None, L.ACT["relu"], 0.0,
                                                           R, S_, L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(g[3]), L.ptr(d_raw), L.ptr(d_rows), None, 0,
                                                           L.stream_ptr())
    L.check(call(G, S), "evd_raw2outputs_feat_bwd")
    torch.cuda.synchronize()
    r = P.feat_reference(c, DEV)
    assert (d_raw[..., :4] == 0).all() and (d_raw[..., 5] == 0).all()
    check("C6 d_sigma", d_raw[..., 4], r["d_sigma"], r["E_d_sigma"])
    check("C6 d_rows", d_rows, r["d_rows"], r["E_d_rows"])
    for G_, S_ in ((0, S), (129, S), (G, 257), (G, 0)):
        with pytest.raises(L.EvdError):
            L.check(call(G_, S_), "evd_raw2outputs_feat_bwd")


# ---- the per-ray colour network ---------------------------------------------------------------------------------------------------
_NETS = {}


def level(Lv, bias):
    from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures
    if (Lv, bias) not in _NETS:
        d = V.DIMS["coarse"]
        _NETS[(Lv, bias)] = VoxelNeRFRayFeatures(V._state_dict("coarse", (10, Lv), bias), "", V.AABB, num_layers=2, hidden_dim=64, geo_feat_dim=15,
                                                 num_layers_color=3, input_ch=d["FT"] + 63, multires=10, multires_views=Lv, app_dim=32,
                                                 app_n_comp=(64, 16, 16), n_voxels=d["nvox"], rgb_activate="relu", composite_feature=True,
                                                 precision="f16x3")
    return _NETS[(Lv, bias)]


def run_color(c, net, a, fill=None):
    """-> colour, d_map, d_viewdirs | None, {w0.. b2: gradient | None}"""
    R, st = c["R"], c["stride"]
    fmap, rays, g_color = dev(a["fmap"]), dev(a["rays"]), dev(a["g_color"])
    vd = C.c_void_p(rays.data_ptr() + 4 * a["col"])
    lib, h = L.lib(), net._h
    nb = int(lib.evd_voxel_color_rows_store_bytes(h, R))
    assert nb > 0
    store = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    color = torch.full((R, 3), float("nan"), device=DEV)
    L.check(lib.evd_voxel_color_rows_train(h, L.ptr(fmap), vd, st, R, L.ptr(color), L.ptr(store), nb, L.stream_ptr()), "evd_voxel_color_rows_train")
    nin = 15 + 3 * (1 + 2 * c["Lv"])
    shapes = dict(w0=(64, nin), b0=(64,), w1=(64, 64), b1=(64,), w2=(3, 64), b2=(3,))
    base = {k: (torch.full(sh, float("nan"), device=DEV) if fill is None else fill[k].clone()) for k, sh in shapes.items()}
    gs = L.VoxelGrads()
    gs.accumulate = int(fill is not None)
    for l in range(3):
        gs.color_w[l] = base[f"w{l}"].data_ptr()
        gs.color_b[l] = base[f"b{l}"].data_ptr() if c["bias"] else None
    d_map = torch.full((R, 15), float("nan"), device=DEV)
    d_vd = torch.full((R, 3), float("nan"), device=DEV) if c["want_dirs"] else None
    nw = int(lib.evd_voxel_color_rows_backward_workspace_bytes(h, R))
    ws = torch.empty((nw,), dtype=torch.uint8, device=DEV)
    L.check(lib.evd_voxel_color_rows_backward(h, L.ptr(g_color), L.ptr(fmap), vd, st, R, L.ptr(store), nb, C.byref(gs), L.ptr(d_map), L.ptr(d_vd),
                                              L.ptr(ws), nw, L.stream_ptr()), "evd_voxel_color_rows_backward")
    torch.cuda.synchronize()
    return color, d_map, d_vd, base


@pytest.mark.parametrize("c", P.COLOR_CASES, ids=[c["id"] for c in P.COLOR_CASES])
def test_color_rows_match_float64(c):
    net, a = level(c["Lv"], c["bias"]), P.color_inputs(c)
    keep = torch.as_tensor(~a["unsure"]).to(DEV)
    assert int((~keep).sum()) <= P.UNSURE_CAP * c["R"]
    fill = None
    if c["accumulate"]:
        g = torch.Generator(device=DEV).manual_seed(c["R"])
        nin = 15 + 3 * (1 + 2 * c["Lv"])
        fill = {k: torch.randn(sh, generator=g, device=DEV) for k, sh in dict(w0=(64, nin), b0=(64,), w1=(64, 64), b1=(64,), w2=(3, 64), b2=(3,)).items()}
    color, d_map, d_vd, grads = run_color(c, net, a, fill)
    r = P.color_reference(c, DEV)
    check(f"{c['id']} color", color, r["color"], r["E_color"], keep)
    check(f"{c['id']} d_map", d_map, r["d_map"], r["E_d_map"], keep)
    if c["want_dirs"]:
        check(f"{c['id']} d_dirs", d_vd, r["d_dirs"], r["E_d_dirs"], keep)
    for k, gk in grads.items():
        if k.startswith("b") and not c["bias"]:
            assert torch.isnan(gk).all() if fill is None else torch.equal(gk, fill[k]), f"{k}: written through a NULL gradient pointer"
            continue
        ref, E = r["d_" + k], r["E_d_" + k]
        if fill is not None:                                # the kernel adds its sum to the caller's value: one more float32 add
            ref, E = ref + fill[k].double(), E + (ref + fill[k].double()).abs()
        check(f"{c['id']} d_{k}", gk, ref, E)


@pytest.mark.parametrize("Lv,bias", [(4, True), (3, False)])
def test_color_rows_forward_is_the_inference_pass_bit_for_bit(Lv, bias):
    """evd_voxel_forward on the composite level returns the composited map and the colour it computed from it"""
    net = level(Lv, bias)
    c = V.case("composite", "coarse", "f16x3", 70, 33, "forward", bias=bias, enc=(10, Lv), composite_feature=True, rgb_activate="relu")
    t = {k: dev(v) for k, v in V.inputs(c).items()}
    color, _, _, _, fmap = net.forward(t["pts"], t["vd"], t["fts"], t["z"], t["rd"], precision="f16x3")
    R = 70
    nb = int(L.lib().evd_voxel_color_rows_store_bytes(net._h, R))
    store = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    out = torch.full((R, 3), float("nan"), device=DEV)
    L.check(L.lib().evd_voxel_color_rows_train(net._h, L.ptr(fmap), L.ptr(t["vd"]), 3, R, L.ptr(out), L.ptr(store), nb, L.stream_ptr()), "train")
    torch.cuda.synchronize()
    assert torch.equal(out, color)


def test_color_rows_backward_is_bit_reproducible():
    c = [k for k in P.COLOR_CASES if k["R"] == 257 and k["Lv"] == 4 and k["bias"]][0]
    net, a = level(c["Lv"], c["bias"]), P.color_inputs(c)
    one, two = run_color(c, net, a), run_color(c, net, a)
    assert torch.equal(one[1], two[1])
    for k in one[3]:
        assert torch.equal(one[3][k], two[3][k]), k


def test_color_rows_refuse_other_levels():
    from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures, VoxelNeRFSampleFeatures
    d = V.DIMS["coarse"]
    plain = VoxelNeRFRayFeatures(V._state_dict("coarse", (10, 4), True), "", V.AABB, num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3,
                                 input_ch=d["FT"] + 63, multires=10, multires_views=4, app_dim=32, app_n_comp=(64, 16, 16), n_voxels=d["nvox"])
    f = V.DIMS["fine"]
    wide = VoxelNeRFSampleFeatures(V._state_dict("fine", (10, 4), True), "", V.AABB, num_layers=2, hidden_dim=256, geo_feat_dim=128, num_layers_color=3,
                                   input_ch=f["FT"] + 63, multires=10, multires_views=4, app_dim=32, app_n_comp=(64, 16, 16), n_voxels=f["nvox"],
                                   composite_feature=True)
    x = torch.zeros((4, 128), device=DEV)
    for net, word in ((plain, b"composite_feature"), (wide, b"standard coarse level")):
        assert L.lib().evd_voxel_color_rows_store_bytes(net._h, 4) == 0
        rc = L.lib().evd_voxel_color_rows_train(net._h, L.ptr(x), L.ptr(x), 3, 4, L.ptr(x), L.ptr(x), 4096, L.stream_ptr())
        assert rc != 0 and word in L.lib().evd_last_error()


def test_zz_print_shares():
    print("worst error / bound by output: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(SHARES.items())))
