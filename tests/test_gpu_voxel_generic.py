"""The PDRF level of any width, depth and geo size (csrc/kernel_voxel_generic.hip; evd_voxel_create accepts hidden 64 / 128 / 256, geo
1..128, 1..4 + 1..4 layers, 16..64 feature channels) against the float64 restatement of tests/voxel_generic_ref.py, itself pinned to the
reference's class by golden G41.  Inference: evd_voxel_mlp, evd_voxel_forward, NeRFAll.render_rays of a c2f model whose two levels are
generic.  Every case fails on a library that refuses these shapes (evd_voxel_create raises).  Training: tests/test_gpu_voxel_generic_train.py.

Bounds (voxel_generic_ref.bounds, fixed from the float64 evaluations before the kernel runs): raw and the geo rows within
F32_GRADE max(1, A) = 5e-5 max(1, A) in f32 / f16x3 / f16c, 4 E_q + that floor in f16 / bf16.  Composited outputs take voxel_level_ref's
floor F (1 + 2 D) max(1, V).  The measured worst errors are printed by every test.

Measured on one MI355X (worst over the eight runs; the range of the bounds in brackets): f32 raw 2.8e-7, geo rows 3.7e-7 [7.0e-5 .. 8.8e-5];
f16x3 raw 1.5e-7, geo rows 1.7e-7 [the same]; f16 raw 3.0e-4, geo rows 3.7e-4 [3.3e-4 .. 1.6e-3, each run at about a quarter of its own];
bf16 raw 2.2e-3, geo rows 2.8e-3 [2.2e-3 .. 1.1e-2, likewise].  evd_voxel_forward: colour 1.2e-7, weights 2.4e-7 [5.9e-4];
c2f render of two generic levels: rgb0 1.1e-7, rgb 1.7e-7 [1.9e-4]; standard coarse + generic fine: 1.1e-7, 1.4e-7."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import voxel_generic_ref as G

pytestmark = pytest.mark.gpu

MODES = ("f32", "f16x3", "f16", "bf16")
_NETS, _EXACT = {}, {}


def level(name, sd=None):
    """the library's level of a case (cached for the case's own state dict)"""
    from evdeblurnerf_amd.voxnerf import VoxelNeRFSampleFeatures
    HD, Gd, FT, NS, NC, L, Lv, bias, R, S = G.CASES[name]
    key = G.CASES[name][:8]
    if sd is not None or key not in _NETS:
        net = VoxelNeRFSampleFeatures(sd if sd is not None else G.case_state_dict(name), "", G.AABB, multires=L, multires_views=Lv, app_dim=32,
                                      app_n_comp=(64, 16, 16), n_voxels=G.NVOX, precision="f16x3", **G.case_kwargs(name))
        if sd is not None:
            return net
        _NETS[key] = net
    return _NETS[key]


def exact(name):
    if name not in _EXACT:
        _EXACT[name] = G.evaluate(name, "cuda")
    return _EXACT[name]


def run(name, mode, net=None):
    a = {k: torch.tensor(v, device="cuda") for k, v in G.case_inputs(name).items()}
    raw, geo = (net or level(name)).mlpforward(a["pts"], a["vd"], a["fts"], precision=mode, want_feature=True)
    torch.cuda.synchronize()
    R, S = G.CASES[name][-2:]
    assert raw.shape == (R, S, 4) and geo.shape == (R, S, G.CASES[name][1])
    return raw.reshape(-1, 4), geo.reshape(R * S, -1)


@pytest.fixture(scope="module", autouse=True)
def _clear():
    yield
    _NETS.clear()
    _EXACT.clear()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(G.CASES))
def test_inference_vs_float64(name, mode):
    ex, bound, e_q = G.bounds(name, mode, "cuda", exact=exact(name))
    raw, geo = run(name, mode)
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(geo).all())
    e_raw, e_geo = float((raw.double() - ex["raw"]).abs().max()), float((geo.double() - ex["geo"]).abs().max())
    print(f"[{name} {mode}] raw {e_raw:.3e}, geo rows {e_geo:.3e}, bound {bound:.3e} (A {ex['A']:.2f}, model error {e_q:.1e})")
    assert e_raw <= bound and e_geo <= bound


@pytest.mark.parametrize("mode", MODES)
def test_widest_level_with_the_deepest_colour_net(mode):
    """256 / 128 / 64 with 2 + 4 layers and colour biases: the largest bias block (512 zeros + 3 x 256 + 32 floats) and the 256-wide body
    that walks the colour layer count at run time; not in CASES (golden G41 pins those), the float64 side is the same restatement"""
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.voxnerf import VoxelNeRFSampleFeatures
    HD, Gd, FT, NS, NC, R, S = 256, 128, 64, 2, 4, 50, 21
    key = ("wide", HD, Gd, FT, NS, NC)
    sd = W.make_pdrf_state_dict(71, W.pdrf_grid_size(G.AABB[0], G.AABB[1], G.NVOX), input_ch=FT + 63, num_layers=NS, hidden_dim=HD, geo_feat_dim=Gd,
                                num_layers_color=NC, add_bias_color=True)
    if key not in _NETS:
        _NETS[key] = VoxelNeRFSampleFeatures(sd, "", G.AABB, app_dim=32, app_n_comp=(64, 16, 16), n_voxels=G.NVOX, precision="f16x3", num_layers=NS,
                                             hidden_dim=HD, geo_feat_dim=Gd, num_layers_color=NC, input_ch=FT + 63)
    a = {k: torch.tensor(v, device="cuda") for k, v in G._inputs(FT, R, S).items()}
    raw, geo = _NETS[key].mlpforward(a["pts"], a["vd"], a["fts"], precision=mode, want_feature=True)
    P = {k: torch.tensor(np.asarray(v), device="cuda", dtype=torch.float64) for k, v in sd.items() if k.startswith(("sigma_net.", "color_net."))}
    args = (a["pts"].double().reshape(-1, 3), a["vd"].double()[:, None].expand(R, S, 3).reshape(-1, 3), a["fts"].double().reshape(-1, FT), 10, 4)
    raw64, geo64, pre = G.level_forward64(P, *args)
    A = max(float(y.abs().max()) for _, y in pre)
    bound = G.F32_GRADE * max(1.0, A)
    if mode in G.QUANT:
        rq, gq, _ = G.level_forward64(P, *args, quant=mode)
        bound += 4 * max(float((rq - raw64).abs().max()), float((gq - geo64).abs().max()))
    e_raw, e_geo = float((raw.reshape(-1, 4).double() - raw64).abs().max()), float((geo.reshape(-1, Gd).double() - geo64).abs().max())
    print(f"[256 / 128 / 64, 2 + 4 layers, biases, {mode}] raw {e_raw:.3e}, geo rows {e_geo:.3e}, bound {bound:.3e} (A {A:.2f})")
    assert e_raw <= bound and e_geo <= bound


@pytest.mark.parametrize("name", ["w64_g7_1p1", "w256_g100_2p2", "w128_g32_2p3_s33"])
def test_f16c_is_f16x3_and_rows_are_optional(name):
    """EVD_PREC_F16C on a generic level runs the split-float16 kernel: the same bits.  raw does not depend on whether the rows are written"""
    raw_c, geo_c = run(name, "f16c")
    raw_x, geo_x = run(name, "f16x3")
    assert torch.equal(raw_c.view(torch.int32), raw_x.view(torch.int32)) and torch.equal(geo_c.view(torch.int32), geo_x.view(torch.int32))
    a = {k: torch.tensor(v, device="cuda") for k, v in G.case_inputs(name).items()}
    raw_n, none = level(name).mlpforward(a["pts"], a["vd"], a["fts"], precision="f16x3", want_feature=False)
    assert none is None and torch.equal(raw_n.reshape(-1, 4).view(torch.int32), raw_x.view(torch.int32))


def test_geo_rows_stop_at_g_columns():
    """G = 100 leaves 28 padded channels in the last geo tile: the row buffer's next row (and the 400 bytes behind the last row) stay as they were"""
    import evdeblurnerf_amd._lib as L
    name = "w256_g100_2p2"
    net = level(name)
    a = {k: torch.tensor(v, device="cuda") for k, v in G.case_inputs(name).items()}
    R, S, Gd = 50, 21, 100
    raw = torch.empty((R, S, 4), device="cuda")
    buf = torch.full((R * S * Gd + Gd,), -7.0, device="cuda")
    vd = a["vd"].contiguous()
    L.check(L.lib().evd_voxel_mlp(net._h, L.PREC["f32"], L.ptr(a["pts"]), L.ptr(vd), 3, L.ptr(a["fts"]), a["fts"].shape[-1], R, S, L.ptr(raw), L.ptr(buf),
                                  L.stream_ptr()), "evd_voxel_mlp")
    torch.cuda.synchronize()
    assert bool((buf[R * S * Gd:] == -7.0).all())
    ex = exact(name)
    assert float((buf[:R * S * Gd].reshape(-1, Gd).double() - ex["geo"]).abs().max()) <= G.F32_GRADE * max(1.0, ex["A"])


@pytest.mark.parametrize("name", ["w128_g31_3p4", "w64_g15_3p3_enc6_2_bias"])
def test_load_params_equals_a_fresh_handle(name):
    """after evd_voxel_load_params with new parameters (the device re-pack of the generic stream and of the bias block) every mode gives
    the bits of a handle created from them"""
    net = level(name, sd=G.case_state_dict(name))          # a handle of its own: it is re-loaded below
    other = G.case_state_dict(name, seed=G.SEEDS[name] + 20)
    keys = G.net_keys(name)
    assert [k for k, _, _ in net.param_blocks() if k in other] == keys       # the reference's names, in its order (absent biases are not parameters)
    flat = net.flat_params(other)
    assert flat.numel() == sum(int(np.prod(s)) for _, s, _ in net.param_blocks())
    net.load_params(flat)
    fresh = level(name, sd=other)
    for mode in MODES:
        a, b = run(name, mode, net=net), run(name, mode, net=fresh)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), mode
    ex = run(name, "f32")
    assert float((ex[0] - run(name, "f32", net=net)[0]).abs().max()) > 1e-3        # the new parameters are different ones


@pytest.mark.parametrize("name", ["w128_g31_3p4", "w256_g128_ft16_4p2"])
def test_level_forward_entry(name):
    """VoxelNeRFBase.forward (evd_voxel_forward) on a generic level: the feature rows are evd_voxel_mlp's bit for bit, colour, depth, acc
    and weights within voxel_level_ref's composited floor of the float64 composition"""
    import voxel_level_ref as V
    HD, Gd, FT, NS, NC, L, Lv, bias, R, S = G.CASES[name]
    net, ex = level(name), exact(name)
    rs = np.random.RandomState(5)
    z = np.sort(rs.uniform(0, 1, (R, S)).astype(np.float32), -1)
    rd = rs.normal(size=(R, 3)).astype(np.float32)
    a = {k: torch.tensor(v, device="cuda") for k, v in G.case_inputs(name).items()}
    zt, rdt = torch.tensor(z, device="cuda"), torch.tensor(rd, device="cuda")
    color, depth, acc, wts, feat = net.forward(a["pts"], a["vd"], a["fts"], zt, rdt, precision="f16x3")
    torch.cuda.synchronize()
    assert torch.equal(feat.reshape(R * S, -1).view(torch.int32), run(name, "f16x3")[1].view(torch.int32))
    ref = V.level_outputs64(ex["raw"], ex["geo"], zt, rdt, dict(rgb_activate="none", sigma_activate="relu"))
    D = float(((zt[:, -1] - zt[:, 0]).double() * rdt.double().norm(dim=-1)).max())
    F = G.F32_GRADE * max(1.0, ex["A"]) * (1 + 2 * D)
    for k, got, vmax in (("color", color, 1.0), ("depth", depth, 1.0), ("acc", acc, 1.0), ("weights", wts, 1.0)):
        e, b = float((got.double() - ref[k]).abs().max()), F * vmax + ref["E"][k]
        print(f"[{name} forward] {k}: error {e:.3e}, bound {b:.3e}")
        assert e <= b


def test_c2f_render_of_two_generic_levels():
    """NeRFAll.render_rays, mode='c2f': coarse 128 / 20 / 32 with 3 + 2 layers on 24^3 voxels, fine 128 / 40 / 48 (app_dim 16) with 1 + 4
    layers on 48^3, 32 rays, 16 + 16 samples.  The float64 side is the restatement composed as render_rays composes the levels
    (torch_restatement.c2f_pipeline: float64 grid_sample features, level networks, compositing), first AT THE KERNEL'S sample positions
    (every ray), then with importance samples of its own from the float64 coarse weights, on the rays whose merged samples agree to 5e-5
    (G9's rule); rgb0 and rgb within F32_GRADE max(1, A) (1 + 2 D)."""
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.renderer import NeRFAll
    from torch_restatement import c2f_pipeline
    a = W.blurfactory_args(16, coarse_voxels=24 ** 3, fine_voxels=48 ** 3)
    a.coarse_num_layers, a.coarse_num_layers_color, a.coarse_hidden_dim, a.kernel_feat_cnl = 3, 2, 128, 20
    a.fine_num_layers, a.fine_num_layers_color, a.fine_hidden_dim, a.fine_geo_feat_dim, a.fine_app_dim = 1, 4, 128, 40, 16
    gc, gf = W.pdrf_grid_size(*W.BLURFACTORY_AABB, 24 ** 3), W.pdrf_grid_size(*W.BLURFACTORY_AABB, 48 ** 3)
    sdc = W.make_pdrf_state_dict(81, gc, input_ch=32 + 63, num_layers=3, hidden_dim=128, geo_feat_dim=20, num_layers_color=2)
    sdf = W.make_pdrf_state_dict(82, gf, input_ch=48 + 63, num_layers=1, hidden_dim=128, geo_feat_dim=40, num_layers_color=4, app_dim=16)
    sd = dict(W.prefixed(sdc, "mlp_coarse"))
    sd.update(W.prefixed(sdf, "mlp_fine"))
    model = NeRFAll(a, sd, precision="f16x3").eval()
    R, S, Ni, near, far = 32, 16, 16, 0.1, 0.7
    rs = np.random.RandomState(3)
    o = rs.uniform(-0.2, 0.2, (R, 3))
    d = rs.normal(size=(R, 3))
    d *= rs.uniform(0.8, 1.2, (R, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)
    rb = np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far), d / np.linalg.norm(d, axis=-1, keepdims=True)], -1).astype(np.float32)
    ret = model.render_rays(torch.tensor(rb, device="cuda"), S, retraw=True, N_importance=Ni, perturb=0., raw_noise_std=0.)
    torch.cuda.synchronize()
    z0, zm = ret["z_vals0"].cpu().double(), ret["z_vals"].cpu().double()
    assert zm.shape == (R, S + Ni) and bool((zm[:, 1:] >= zm[:, :-1]).all())
    A = [0.0]

    def net64(sdl):
        P = {k: torch.tensor(v, dtype=torch.float64) for k, v in sdl.items() if k.startswith(("sigma_net.", "color_net."))}

        def f(pts, dirs, fts):
            raw, _, pre = G.level_forward64(P, pts, dirs, fts, 10, 4)
            A[0] = max(A[0], max(float(y.abs().max()) for _, y in pre))
            return raw
        return f

    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    grids = {n: ([t64(s[f"app_plane.{i}"]) for i in range(3)], [t64(s[f"app_line.{i}"]) for i in range(3)], t64(s["basis_mat.weight"]))
             for n, s in (("coarse", sdc), ("fine", sdf))}
    with torch.no_grad():
        rgb0, rgb = c2f_pipeline({"coarse": net64(sdc), "fine": net64(sdf)}, grids, t64(rb), z0, zm, W.BLURFACTORY_AABB)
    D = (far - near) * float(np.linalg.norm(d, axis=-1).max())
    bound = G.F32_GRADE * max(1.0, A[0]) * (1 + 2 * D)
    e0, e1 = float((ret["rgb0"].cpu().double() - rgb0).abs().max()), float((ret["rgb_map"].cpu().double() - rgb).abs().max())
    print(f"[c2f render, two generic levels] rgb0 {e0:.3e}, rgb {e1:.3e}, bound {bound:.3e} (A {A[0]:.2f}, D {D:.2f})")
    assert float(rgb.std()) > 1e-3 and e0 <= bound and e1 <= bound
    # The importance samples drawn from the generic coarse level's weights, independently (G9's rule): the float64 coarse weights at the
    # stratified z -> composite_ref.sample_pdf_merge + merge; the images are compared on the rays whose merged samples agree to 5e-5
    from composite_ref import merge, sample_pdf_merge
    from torch_restatement import torch_appfeature, vox_composite
    z0r = (near * (1 - torch.linspace(0, 1, S)) + far * torch.linspace(0, 1, S)).float().expand(R, S)
    assert float((z0r.double() - z0).abs().max()) < 1e-6
    rbt = t64(rb)
    with torch.no_grad():
        pts0 = (rbt[:, None, 0:3] + rbt[:, None, 3:6] * z0r.double()[..., None]).reshape(-1, 3)
        raw0 = net64(sdc)(pts0, rbt[:, None, 8:11].expand(-1, S, -1).reshape(-1, 3), torch_appfeature(*grids["coarse"], pts0, W.BLURFACTORY_AABB))
        _, w0 = vox_composite(raw0.reshape(R, S, 4), z0r.double(), rbt[:, 3:6])
        zs = sample_pdf_merge(z0r, w0.float(), Ni, det=True)["z_samples"]
        zmr, _ = merge(z0r, zs.float())
        same = np.abs(zmr.astype(np.float64) - zm.numpy()).max(-1) < 5e-5
        rgb0i, rgbi = c2f_pipeline({"coarse": net64(sdc), "fine": net64(sdf)}, grids, rbt, z0r.double(), t64(zmr), W.BLURFACTORY_AABB)
    ei = float((ret["rgb_map"].cpu().double() - rgbi).abs()[torch.tensor(same)].max())
    print(f"[c2f render, own importance samples] merged samples agree on {same.mean():.0%} of the rays, rgb there {ei:.3e}, bound {bound:.3e}")
    assert same.mean() > 0.8 and ei <= bound
    # EVD_PREC_F16C on generic levels is EVD_PREC_F16X3, grids included: the same image bit for bit
    ret_c = NeRFAll(a, sd, precision="f16c").eval().render_rays(torch.tensor(rb, device="cuda"), S, retraw=True, N_importance=Ni, perturb=0., raw_noise_std=0.)
    for k in ("rgb_map", "rgb0", "z_vals", "weights"):
        assert torch.equal(ret_c[k].view(torch.int32), ret[k].view(torch.int32)), k
    # a standard level and a generic one in one model: the coarse level of the shipped shape in front of the same fine level
    b = W.blurfactory_args(16, coarse_voxels=24 ** 3, fine_voxels=48 ** 3)
    b.fine_num_layers, b.fine_num_layers_color, b.fine_hidden_dim, b.fine_geo_feat_dim, b.fine_app_dim = 1, 4, 128, 40, 16
    sds = W.make_pdrf_state_dict(83, gc, input_ch=32 + 63, hidden_dim=64, geo_feat_dim=15)
    sd2 = dict(W.prefixed(sds, "mlp_coarse"))
    sd2.update(W.prefixed(sdf, "mlp_fine"))
    mixed = NeRFAll(b, sd2, precision="f16x3").eval()
    ret2 = mixed.render_rays(torch.tensor(rb, device="cuda"), S, retraw=True, N_importance=Ni, perturb=0., raw_noise_std=0.)
    grids["coarse"] = ([t64(sds[f"app_plane.{i}"]) for i in range(3)], [t64(sds[f"app_line.{i}"]) for i in range(3)], t64(sds["basis_mat.weight"]))
    with torch.no_grad():
        rgb0, rgb = c2f_pipeline({"coarse": net64(sds), "fine": net64(sdf)}, grids, t64(rb), ret2["z_vals0"].cpu().double(), ret2["z_vals"].cpu().double(),
                                 W.BLURFACTORY_AABB)
    e0, e1 = float((ret2["rgb0"].cpu().double() - rgb0).abs().max()), float((ret2["rgb_map"].cpu().double() - rgb).abs().max())
    print(f"[c2f render, standard coarse + generic fine] rgb0 {e0:.3e}, rgb {e1:.3e}, bound {bound:.3e}")
    assert e0 <= bound and e1 <= bound
    # such a model trains in f16x3 alone (tests/test_gpu_voxel_generic_train.py): another training precision is refused before anything is created
    import evdeblurnerf_amd._lib as L
    assert model.mlp_coarse.is_standard_shape() is False and mixed.mlp_coarse.is_standard_shape() is True
    for m, s in ((NeRFAll(a, sd, precision="f16"), sd), (NeRFAll(b, sd2, precision="f16"), sd2)):
        with pytest.raises(L.EvdError, match="f16x3"):
            m.enable_training(s)


def _try_create(**over):
    from evdeblurnerf_amd.voxnerf import VoxelNeRFSampleFeatures
    kw = dict(num_layers=2, hidden_dim=128, geo_feat_dim=32, num_layers_color=3, ft=32, composite_feature=False)
    kw.update(over)
    ft = kw.pop("ft")
    from evdeblurnerf_amd import weights as W
    gsz = W.pdrf_grid_size(G.AABB[0], G.AABB[1], G.NVOX)
    sd = W.make_pdrf_state_dict(7, gsz, input_ch=ft + 63, num_layers=kw["num_layers"], hidden_dim=kw["hidden_dim"], geo_feat_dim=kw["geo_feat_dim"],
                                num_layers_color=kw["num_layers_color"])
    return VoxelNeRFSampleFeatures(sd, "", G.AABB, input_ch=ft + 63, app_dim=32, app_n_comp=(64, 16, 16), n_voxels=G.NVOX, precision="f16x3", **kw)


@pytest.mark.parametrize("over,word", [(dict(hidden_dim=96), "hidden_dim 64, 128 or 256"), (dict(geo_feat_dim=129), "geo_feat_dim 1..128"),
                                       (dict(num_layers=5), "1..4"), (dict(num_layers_color=5), "1..4"), (dict(ft=24), "multiple of 16"),
                                       (dict(ft=80), "16..64"), (dict(composite_feature=True), "composite_feature")])
def test_shapes_outside_the_ranges_are_refused_with_the_ranges(over, word):
    import evdeblurnerf_amd._lib as L
    assert _try_create() is not None          # the base shape of this table is accepted
    with pytest.raises(L.EvdError, match=word):
        _try_create(**over)


def test_awp_consumer_refuses_another_geo_width():
    """the AWP sample embedding reads 128 geo channels: rows of a fine level with geo_feat_dim = 100 are refused with a message (they
    are not re-cut into 128-wide rows), so is a NeRFAll whose fine level has another width than its fused consumer; the rows of a generic
    level with geo_feat_dim = 128 are taken"""
    import evdeblurnerf_amd._lib as L
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.awp import SampleFeatureEmbed
    from evdeblurnerf_amd.renderer import NeRFAll
    sd = W.make_awp_embed_state_dict(5)
    ws = [sd[f"sample_feature_embed_layer.{l}.weight"] for l in range(4)]
    bs = [sd[f"sample_feature_embed_layer.{l}.bias"] for l in range(4)]
    embed = SampleFeatureEmbed(ws, bs, precision="f16")
    flat = torch.cat([torch.as_tensor(t).reshape(-1) for pair in zip(ws, bs) for t in pair]).cuda()
    geo100 = run("w256_g100_2p2", "f16x3")[1]
    with pytest.raises(L.EvdError, match="128 geo channels"):
        embed(flat, geo100)
    with pytest.raises(L.EvdError, match="128 geo channels"):
        embed(flat, geo100[:128].reshape(1, 128, 100))      # 12800 floats would re-cut into exactly 100 rows of 128
    h = embed(flat, run("w256_g128_ft16_4p2", "f16x3")[1])
    torch.cuda.synchronize()
    assert h.shape == (1050, 64) and bool(torch.isfinite(h).all())
    a = W.blurfactory_args(16, coarse_voxels=24 ** 3, fine_voxels=48 ** 3, use_awp=True)
    a.fine_geo_feat_dim = 40
    gc, gf = W.pdrf_grid_size(*W.BLURFACTORY_AABB, 24 ** 3), W.pdrf_grid_size(*W.BLURFACTORY_AABB, 48 ** 3)
    sdm = dict(W.prefixed(W.make_pdrf_state_dict(83, gc, input_ch=95), "mlp_coarse"))
    sdm.update(W.prefixed(W.make_pdrf_state_dict(84, gf, input_ch=127, hidden_dim=256, geo_feat_dim=40), "mlp_fine"))
    with pytest.raises(L.EvdError, match="fine_geo_feat_dim = 40"):
        NeRFAll(a, sdm, awpnet=SimpleNamespace(embed=embed), precision="f16x3")
