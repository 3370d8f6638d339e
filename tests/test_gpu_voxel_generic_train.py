"""Training of a PDRF level of any width, depth and geo size (the generic path of evd_voxel_mlp_train / _backward, EVD_PREC_F16X3:
csrc/kernel_voxel_generic.hip TRAIN, csrc/kernel_voxel_train_generic.hip) against float64 autograd of the restatement of
tests/voxel_generic_ref.py, itself pinned to the reference's class by golden G41.  Every test fails on a library that refuses these shapes.

ReLU ties: a unit whose float64 pre-activation lies within TAU = 2e-6 of zero is decided by rounding in any float32-grade arithmetic, so
d raw (and the gradient that arrives at the geo rows) is zero on the samples that have one -- at most 10 % of a case, asserted on the CPU
in tests/test_voxel_generic_ref.py; through NeRFAll, where a ray's colour reaches all its samples, the loss weight of every RAY that carries
a tie sample is zero, under the same cap.  Bounds (tests/test_gpu_train_f32grade.py, the project's for this mode): parameter gradients
5e-6 relative L2, gradients to fts, pts, viewdirs and from d_feature 2e-4.  Every test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest
import torch

import voxel_generic_ref as G
from evdeblurnerf_amd import weights as W
from test_gpu_train import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS = {}


def level(name):
    from evdeblurnerf_amd.voxnerf import VoxelNeRFSampleFeatures
    HD, Gd, FT, NS, NC, L, Lv, bias, R, S = G.CASES[name]
    key = G.CASES[name][:8]
    if key not in _NETS:
        _NETS[key] = VoxelNeRFSampleFeatures(G.case_state_dict(name), "", G.AABB, multires=L, multires_views=Lv, app_dim=32, app_n_comp=(64, 16, 16),
                                             n_voxels=G.NVOX, precision="f16x3", **G.case_kwargs(name))
    return _NETS[key]


@pytest.fixture(scope="module", autouse=True)
def _clear():
    yield
    _NETS.clear()


def T(x):
    return torch.tensor(x, device=DEV)


def inputs(name):
    return {k: T(v) for k, v in G.case_inputs(name).items()}


@pytest.mark.parametrize("name", list(G.CASES))
def test_training_forward_is_the_inference_arithmetic(name):
    net, a = level(name), inputs(name)
    raw, store, geo = net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16x3", want_feature=True)
    raw_i, geo_i = net.mlpforward(a["pts"], a["vd"], a["fts"], precision="f16x3", want_feature=True)
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int32), raw_i.view(torch.int32)) and torch.equal(geo.view(torch.int32), geo_i.view(torch.int32))
    raw_n, _, none = net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16x3")
    assert none is None and torch.equal(raw_n.view(torch.int32), raw_i.view(torch.int32))


@pytest.mark.parametrize("name", list(G.CASES))
def test_parameter_gradients_match_float64_autograd(name):
    net, a = level(name), inputs(name)
    ex = G.evaluate(name, DEV, grads=True)
    frac = float(ex["tie"].double().mean())
    assert frac <= G.TIE_CAP
    R, S = G.CASES[name][-2:]
    raw, store, _ = net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16x3")
    flat, _, _, _ = net.mlp_backward_flat(ex["d_raw"].float().reshape(R, S, 4), raw, store, precision="f16x3", want_fts=False)
    torch.cuda.synchronize()
    got = {k: v for k, v in net.unflatten(flat).items() if k in ex["grads"] or bool((v != 0).any())}
    assert set(got) == set(G.net_keys(name)) == set(ex["grads"])       # the reference's named_parameters(): an absent bias gets no gradient
    errs = {k: rel_l2(v.double(), ex["grads"][k]) for k, v in got.items()}
    worst = max(errs, key=errs.get)
    print(f"[{name}] worst relative L2 error of a parameter gradient vs float64 autograd (true ReLU, {100 * frac:.1f} % of the samples zeroed as "
          f"ties): {worst} {errs[worst]:.2e}")
    assert errs[worst] < 5e-6, {k: f"{v:.1e}" for k, v in errs.items()}


@pytest.mark.parametrize("name", ["w64_g7_1p1", "w128_g31_3p4", "w256_g100_2p2", "w64_g15_3p3_enc6_2_bias", "w128_g32_2p3_s33"])
def test_gradients_to_the_inputs_and_from_the_geo_rows(name):
    """autograd through mlp_train: d fts, d pts and d viewdirs (through the two encodings), with a gradient arriving at the geo rows"""
    HD, Gd, FT, NS, NC, L, Lv, bias, R, S = G.CASES[name]
    net, sd, a = level(name), G.case_state_dict(name), G.case_inputs(name)
    ex = G.evaluate(name, DEV)
    keep = (~ex["tie"]).double()[:, None]
    d_raw = torch.tensor(a["d_raw"], device=DEV, dtype=torch.float64).reshape(-1, 4) * keep
    d_geo = torch.tensor(np.random.RandomState(31).normal(size=(R * S, Gd)), device=DEV) * keep
    flat = net.flat_params(sd)
    pts, vd, fts = (T(a[k]).requires_grad_(True) for k in ("pts", "vd", "fts"))
    raw, geo = net.mlp_train(flat, pts, vd, fts, "f16x3", want_feature=True)
    ((raw.reshape(-1, 4) * d_raw.float()).sum() + (geo.reshape(-1, Gd) * d_geo.float()).sum()).backward()
    P = {k: torch.tensor(np.asarray(v), device=DEV, dtype=torch.float64, requires_grad=True) for k, v in sd.items() if k.startswith(("sigma_net.", "color_net."))}
    p64, v64, f64 = (torch.tensor(a[k], device=DEV, dtype=torch.float64, requires_grad=True) for k in ("pts", "vd", "fts"))
    rraw, rgeo, _ = G.level_forward64(P, p64.reshape(-1, 3), v64[:, None].expand(R, S, 3).reshape(-1, 3), f64.reshape(-1, FT), L, Lv)
    ((rraw * d_raw).sum() + (rgeo * d_geo).sum()).backward()
    got = net.unflatten(flat.grad)
    errs = {k: rel_l2(got[k].double(), P[k].grad) for k in P}
    errs.update({"fts": rel_l2(fts.grad.double(), f64.grad), "pts (through PE)": rel_l2(pts.grad.double(), p64.grad),
                 "viewdirs (through PE)": rel_l2(vd.grad.double(), v64.grad)})
    print(f"[{name}] relative L2 errors vs float64 autograd with d_feature:", {k: f"{v:.1e}" for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:5]})
    assert max(errs.values()) < 2e-4, errs


@pytest.mark.parametrize("name", ["w128_g31_3p4", "w256_g100_2p2"])
def test_backward_repeats_bit_for_bit_and_accumulates(name):
    net, a = level(name), inputs(name)
    R, S = G.CASES[name][-2:]
    Gd = G.CASES[name][1]
    d_geo = T(np.random.RandomState(32).normal(size=(R, S, Gd)).astype(np.float32))
    runs = []
    for _ in range(2):
        raw, store, _ = net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16x3", want_feature=True)
        runs.append(net.mlp_backward_flat(a["d_raw"], raw, store, precision="f16x3", pts=a["pts"], viewdirs=a["vd"], d_feature=d_geo))
    torch.cuda.synchronize()
    for x, y in zip(*runs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    flat = runs[0][0]
    assert float(flat.abs().max()) > 0 and all(bool(torch.isfinite(x).all()) for x in runs[0])
    known = torch.randn(flat.shape, generator=torch.Generator().manual_seed(3)).to(DEV) * flat.abs().mean()
    buf = known.clone()
    raw, store, _ = net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16x3", want_feature=True)
    assert net.mlp_backward_flat(a["d_raw"], raw, store, precision="f16x3", d_feature=d_geo, accumulate_into=buf, want_fts=False)[0] is None
    assert torch.equal(buf, known + flat)


def test_queries_and_the_other_training_precisions():
    """a generic level trains in f16x3 alone: the store query answers 0 for every other precision and the entries refuse them with a message
    that names f16x3, leaving sentinel-filled outputs as they were; on a standard handle the _net query is evd_voxel_backward_workspace_bytes()
    and the store sizes are the parent's"""
    import evdeblurnerf_amd._lib as L
    lib = L.lib()
    name = "w128_g32_2p3"
    net, a = level(name), inputs(name)
    R, S = G.CASES[name][-2:]
    for prec in ("f16", "bf16", "f16c", "f16m", "f32"):
        assert lib.evd_voxel_train_store_bytes_prec(net._h, L.PREC[prec], R * S) == 0 and lib.evd_voxel_backward_workspace_bytes_net(net._h, L.PREC[prec]) == 0
    nb = lib.evd_voxel_train_store_bytes_prec(net._h, L.PREC["f16x3"], R * S)
    assert nb > 0 and lib.evd_voxel_backward_workspace_bytes_net(net._h, L.PREC["f16x3"]) > 0
    with pytest.raises(L.EvdError, match="f16x3"):
        net.mlpforward_train(a["pts"], a["vd"], a["fts"], precision="f16")
    raw, store = torch.full((R, S, 4), -7.0, device=DEV), torch.full((nb,), 7, dtype=torch.uint8, device=DEV)
    rc = lib.evd_voxel_mlp_train(net._h, L.PREC["f16"], L.ptr(a["pts"]), L.ptr(a["vd"]), 3, L.ptr(a["fts"]), a["fts"].shape[-1], R, S, L.ptr(raw), None,
                                 L.ptr(store), store.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"f16x3" in lib.evd_last_error()
    assert bool((raw == -7.0).all()) and bool((store == 7).all())
    flat = torch.full((sum(int(np.prod(sh)) for _, sh, _ in net.param_blocks()),), -7.0, device=DEV)
    with pytest.raises(L.EvdError, match="f16x3"):
        net.mlp_backward_flat(torch.zeros((R, S, 4), device=DEV), raw, store, precision="f16", accumulate_into=flat)
    gs = L.VoxelGrads()
    gs.sigma_w[0] = flat.data_ptr()
    ws = torch.full((4096,), 7, dtype=torch.uint8, device=DEV)
    rc = lib.evd_voxel_mlp_backward(net._h, L.PREC["f16"], L.ptr(raw), L.ptr(raw), None, None, 0, R, S, L.ptr(store), store.numel(), C.byref(gs), None, 0, None, None, 0, None, None, L.ptr(ws), ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"f16x3" in lib.evd_last_error()
    assert bool((flat == -7.0).all()) and bool((ws == 7).all())
    from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures
    gsz = W.pdrf_grid_size(G.AABB[0], G.AABB[1], G.NVOX)
    std = VoxelNeRFRayFeatures(W.make_pdrf_state_dict(7, gsz, input_ch=95), "", G.AABB, n_voxels=G.NVOX, precision="f16x3")
    assert [k for k, _, _ in std.param_blocks()] == std.PARAM_KEYS
    for prec in ("f16", "bf16", "f16x3", "f16c", "f16m"):
        assert lib.evd_voxel_backward_workspace_bytes_net(std._h, L.PREC[prec]) == lib.evd_voxel_backward_workspace_bytes() > 0
    # the parent's store sizes (csrc/voxel_train.h: 8 tiles per 256 samples; the 64-wide level's f16 tile holds 16 KiB): unchanged
    assert lib.evd_voxel_train_store_bytes_prec(std._h, L.PREC["f16x3"], 1050) == 2 * lib.evd_voxel_train_store_bytes_prec(std._h, L.PREC["f16"], 1050) > 0
    assert lib.evd_voxel_train_store_bytes_prec(std._h, L.PREC["f16"], 1050) == lib.evd_voxel_train_store_bytes(std._h, 1050)
    assert lib.evd_voxel_train_store_bytes_prec(std._h, L.PREC["f32"], 1050) == 0


# ---- through NeRFAll: coarse 128 / 20 / 32 with 3 + 2 layers on 24^3 voxels, fine 128 / 40 / 48 (app_dim 16) with 1 + 4 layers on 48^3
# weight seeds (coarse, fine).  Two generic levels: chosen on the float64 restatement alone, the first of (81, 82) + 10 k for which at most
# 10 % of the 32 rays carry a tie sample (k = 0: 22 %, k = 1: 9.4 %; the next six: 22 .. 44 %).  The mixed model is not compared with float64.
SEEDS = {False: (91, 92), True: (83, 82)}


def _generic_model(fine_only=False, seeds=None, **kw):
    from evdeblurnerf_amd.renderer import NeRFAll
    a = W.blurfactory_args(16, coarse_voxels=24 ** 3, fine_voxels=48 ** 3)
    gc, gf = W.pdrf_grid_size(*W.BLURFACTORY_AABB, 24 ** 3), W.pdrf_grid_size(*W.BLURFACTORY_AABB, 48 ** 3)
    sc, sf = seeds or SEEDS[bool(fine_only)]
    if fine_only:       # the coarse level of the shipped shape in front of a generic fine level
        sdc = W.make_pdrf_state_dict(sc, gc, input_ch=32 + 63, hidden_dim=64, geo_feat_dim=15)
    else:
        a.coarse_num_layers, a.coarse_num_layers_color, a.coarse_hidden_dim, a.kernel_feat_cnl = 3, 2, 128, 20
        sdc = W.make_pdrf_state_dict(sc, gc, input_ch=32 + 63, num_layers=3, hidden_dim=128, geo_feat_dim=20, num_layers_color=2)
    a.fine_num_layers, a.fine_num_layers_color, a.fine_hidden_dim, a.fine_geo_feat_dim, a.fine_app_dim = 1, 4, 128, 40, 16
    sdf = W.make_pdrf_state_dict(sf, gf, input_ch=48 + 63, num_layers=1, hidden_dim=128, geo_feat_dim=40, num_layers_color=4, app_dim=16)
    sd = dict(W.prefixed(sdc, "mlp_coarse"))
    sd.update(W.prefixed(sdf, "mlp_fine"))
    return NeRFAll(a, sd, precision="f16x3", **kw), sd, sdc, sdf


def _rays(R, seed, near=0.1, far=0.7):
    rs = np.random.RandomState(seed)
    o = rs.uniform(-0.2, 0.2, (R, 3))
    d = rs.normal(size=(R, 3))
    d *= rs.uniform(0.8, 1.2, (R, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far), d / np.linalg.norm(d, axis=-1, keepdims=True)], -1).astype(np.float32)


def test_nerfall_parameter_gradients_match_float64_autograd(fine_only=False):
    """render_rays_train of a c2f model with two generic levels, 32 rays, 16 + 16 samples,
    against float64 autograd of the restatement composed as render_rays composes the levels (torch_restatement.c2f_pipeline) on the
    kernel's sample positions.  The loss weight of every ray that carries a tie sample in either level is zero (at most 10 % of the rays).
    Network parameters within 2e-4 of their norm (the composite's float32 d alpha in front of the 5e-6 of the level alone, as
    tests/test_gpu_nerf_generic_train.py states for the NeRF networks), grids within 2e-3 (tests/test_gpu_train_f32grade.py's end-to-end bound)."""
    from torch_restatement import c2f_pipeline
    model, sd, sdc, sdf = _generic_model(fine_only)
    model.train()
    pc, pf = model.trainable_parameters(sd)
    R, S, Ni = 32, 16, 16
    rb_np = _rays(R, 3)
    tgt = np.random.RandomState(5).uniform(0, 1, (R, 3))
    out = model.render_rays_train(T(rb_np), pc, pf, S, Ni)
    zm = out["z_vals"].detach().cpu().double()
    z0 = (0.1 * (1 - torch.linspace(0, 1, S)) + 0.7 * torch.linspace(0, 1, S)).float().expand(R, S).double()       # perturb = 0: the stratified z
    t64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    ties = {}

    def net64(tag, sdl):
        P = {k: t64(v).requires_grad_(True) for k, v in sdl.items() if k.startswith(("sigma_net.", "color_net."))}
        NS, NC = sum(k.startswith("sigma_net.") for k in P), sum(k.startswith("color_net.") and k.endswith("weight") for k in P)

        def f(pts, dirs, fts):
            raw, _, pre = G.level_forward64(P, pts, dirs, fts, 10, 4)
            tie = torch.zeros(raw.shape[0], dtype=torch.bool)
            for n, y in pre:
                if n not in (f"sigma_net.{NS - 1}", f"color_net.{NC - 1}"):
                    tie |= (y.detach().abs() < G.TAU).any(-1)
            ties[(tag, raw.shape[0])] = tie.reshape(R, -1).any(-1)
            return raw
        return f, P

    fc, Pc = net64("coarse", sdc)
    ff, Pf = net64("fine", sdf)
    grids = {n: ([t64(s[f"app_plane.{i}"]).requires_grad_(True) for i in range(3)], [t64(s[f"app_line.{i}"]).requires_grad_(True) for i in range(3)],
                 t64(s["basis_mat.weight"]).requires_grad_(True)) for n, s in (("coarse", sdc), ("fine", sdf))}
    rgb0, rgb = c2f_pipeline({"coarse": fc, "fine": ff}, grids, t64(rb_np), z0, zm, W.BLURFACTORY_AABB)
    tie_rays = torch.stack(list(ties.values())).any(0)
    frac = float(tie_rays.double().mean())
    assert frac <= G.TIE_CAP
    w = (~tie_rays).double()[:, None]
    e0, e1 = float((out["rgb0"].detach().cpu().double() - rgb0.detach()).abs().max()), float((out["rgb_map"].detach().cpu().double() - rgb.detach()).abs().max())
    ((w * (rgb - t64(tgt)) ** 2).sum() + (w * (rgb0 - t64(tgt)) ** 2).sum()).backward()
    wt, tt = w.float().to(DEV), T(tgt.astype(np.float32))
    ((wt * (out["rgb_map"] - tt) ** 2).sum() + (wt * (out["rgb0"] - tt) ** 2).sum()).backward()
    errs, gerrs = {}, {}
    for name, prm, P, lvl in (("coarse", pc, Pc, model.mlp_coarse), ("fine", pf, Pf, model.mlp_fine)):
        got = lvl.unflatten(prm["net"].grad)
        for k in P:
            errs[f"{name}.{k}"] = rel_l2(got[k].cpu().double(), P[k].grad)
        pl, li, ba = grids[name]
        for i in range(3):
            gerrs[f"{name}.plane{i}"] = rel_l2(prm["grids"][i].grad.cpu().double(), pl[i].grad[0].permute(1, 2, 0))
            gerrs[f"{name}.line{i}"] = rel_l2(prm["grids"][3 + i].grad.cpu().double(), li[i].grad[0, :, :, 0].t())
        gerrs[f"{name}.basis"] = rel_l2(prm["grids"][6].grad.cpu().double(), ba.grad)
    worst, gworst = max(errs, key=errs.get), max(gerrs, key=gerrs.get)
    print(f"[NeRFAll generic levels, fine_only={fine_only}] rgb0 {e0:.2e}, rgb {e1:.2e}; worst network gradient {worst} {errs[worst]:.2e}; worst grid "
          f"gradient {gworst} {gerrs[gworst]:.2e}; {100 * frac:.1f} % of the rays zeroed as ties")
    assert e0 < 2e-5 and e1 < 2e-5
    assert errs[worst] < 2e-4, {k: f"{v:.1e}" for k, v in errs.items()}
    assert gerrs[gworst] < 2e-3, {k: f"{v:.1e}" for k, v in gerrs.items()}


@pytest.mark.parametrize("in_place,fine_only", [(False, False), (True, False), (True, True)])
def test_nerfall_training_step(in_place, fine_only):
    """NeRFAll in training mode with two generic levels (fine_only: a standard coarse level in front of a generic fine one), deterministic=True, optim.Adam(model=...): every leaf has the reference's name and
    gets a finite gradient, one iteration from the same state run twice gives the same bits, a few steps lower the loss"""
    from evdeblurnerf_amd import optim as O
    R = 32
    rays = T(W.synthetic_rays(6, R))
    target = torch.full((R, 3), 0.3, device=DEV)
    kw = dict(ndc=True, near=0., far=1., N_samples=16, N_importance=16, perturb=0., raw_noise_std=0.)

    def one(steps):
        model, sd, _, _ = _generic_model(fine_only)
        model.enable_training(sd, grads_in_place=in_place, deterministic=True).train()
        assert {k for k, _ in model.named_parameters()} == set(sd)
        opt = O.Adam(model.parameters(), lr=5e-4, model=model, zero_grads=in_place)
        losses = []
        for _ in range(steps):
            rgb, rgb0, _, _ = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, **kw)
            loss = ((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()
            if not in_place:
                opt.zero_grad()
            loss.backward()
            if len(losses) == 0:
                grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
            opt.step()
            losses.append(float(loss))
        return losses, grads, {k: p.detach().clone() for k, p in model.named_parameters()}

    l1, g1, p1 = one(1)
    l2, g2, p2 = one(6)
    assert all(bool(torch.isfinite(g).all()) for g in g1.values())
    dead = [k for k, g in g1.items() if not bool((g != 0).any())]
    assert not dead, dead
    assert l1[0] == l2[0] and all(torch.equal(g1[k].view(torch.int32), g2[k].view(torch.int32)) for k in g1)
    print(f"[NeRFAll generic levels, grads_in_place={in_place}, standard coarse level={fine_only}] loss over six Adam steps: {l2[0]:.5f} -> {l2[-1]:.5f}")
    assert l2[-1] < l2[0]
