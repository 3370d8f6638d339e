"""The rigid blur kernel network on the device (csrc/kernel_rigid_blur.hip through evdeblurnerf_amd.blurmodel.RigidBlurKernel) against the
float64 restatement tests/rigid_blur_ref.py, on golden G37's three cases, and inside the whole training call of golden G32.

Bounds.  The kernel gets the REFERENCE's own float32 error, as the fixture records it (ref_f32_err: the reference's float32 outputs /
autograd gradients against the same module in float64; max abs for outputs, relative L2 per gradient tensor), times 4 for a different
summation order.  Where a test runs a subset or a multiple of a case's rays, per-tensor records do not carry over; it then uses the case's
output records and the WORST tensor's gradient record (the reference's float32 error level on that network), times 4 again.  For the
whole call the fixture has no float64 twin: new_rays / weight use the reference float32 errors measured at these sizes, 5.1e-7 and 1.9e-8,
times 4, and the kernel's parameter gradients the `side` tolerance tests/test_gpu_train_call.py applies to g.new_rays / g.weight, whose
linear images they are."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import rigid_blur_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0


def _module(c):
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    return RigidBlurKernel.from_state_dict(c["params"], rv_window=c["rv_window"], use_origin=c["use_origin"]).to(DEV)


def _run(mod, c, rays, ids, proj):
    """-> outputs (numpy), {name: gradient}, d rays of the projected sum"""
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    mod.zero_grad(set_to_none=True)
    r = T(rays).requires_grad_(True)
    new_rays, weight, align, extras = mod(400, 400, None, r, {"images_idx": T(ids).reshape(-1, 1)}, return_img_embed=True)
    assert align is None and set(extras) == {"img_embed"}
    loss = (new_rays * T(proj["new_rays"])).sum() + (weight * T(proj["weight"])).sum() + (extras["img_embed"] * T(proj["img_embed"])).sum()
    loss.backward()
    out = {k: v.detach().cpu().numpy() for k, v in dict(new_rays=new_rays, weight=weight, img_embed=extras["img_embed"]).items()}
    return out, {k: p.grad.detach().cpu().numpy().copy() for k, p in mod.named_parameters()}, r.grad.cpu().numpy()


def _subset(c, idx):
    return c["rays"][idx], c["ids"][idx], {k: v[idx] for k, v in c["proj"].items()}


@pytest.mark.parametrize("tag", RR.G37_CASES)
def test_G37_outputs_and_gradients(tag):
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, tag)
    ref = RR.g37_reference(g, tag)
    mod = _module(c)
    assert {k for k, _ in mod.named_parameters()} == set(RR.PARAM_KEYS)
    out, grads, d_rays = _run(mod, c, c["rays"], c["ids"], c["proj"])
    P = c["M"] + int(c["use_origin"])
    assert out["new_rays"].shape == (len(c["ids"]), P, 3, 2) and out["weight"].shape == (len(c["ids"]), c["M"] + 1)
    errs = {k: float(np.abs(out[k] - ref[k]).max()) for k in ("new_rays", "weight")}
    gerr = {k: RR.rel_l2(grads[k], ref["grads"][k]) for k in RR.PARAM_KEYS}
    gerr["rays"] = RR.rel_l2(d_rays, ref["d_rays"])
    for k, e in errs.items():
        print(f"G37 {tag} {k}: {e:.2e} (bound {FACTOR:.0f} x {c['err_out'][k]:.2e})")
    for k, e in gerr.items():
        print(f"G37 {tag} d {k}: {e:.2e} of the norm (bound {FACTOR:.0f} x {c['err_g'][k]:.2e})")
    assert np.array_equal(out["img_embed"], c["params"]["view_embed_module.img_embed"][c["ids"]])
    assert not grads["view_embed_module.img_embed"][RR.ABSENT_IMAGE].any()
    assert np.abs(grads["view_embed_module.img_embed"]).sum(1).astype(bool).sum() == len(set(c["ids"].tolist()))
    for k, e in errs.items():
        assert e <= FACTOR * c["err_out"][k], (k, e)
    for k, e in gerr.items():
        assert e <= FACTOR * c["err_g"][k], (k, e)


def test_per_ray_form_equals_the_table_form():
    """ids == NULL with x = table[ids]: the same outputs and network gradients bit for bit (the same arithmetic on the same rows), and
    d x = the rows whose per-image sums are the table's gradient"""
    from evdeblurnerf_amd.blurmodel import _RigidBlurFn
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, "odd")
    mod = _module(c)
    out, grads, d_rays = _run(mod, c, c["rays"], c["ids"], c["proj"])
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    table = mod.view_embed_module.img_embed.detach()
    ids = T(c["ids"])
    x = table[ids].clone().requires_grad_(True)
    r = T(c["rays"]).requires_grad_(True)
    named = dict(mod.named_parameters())
    net = [named[k] for k in RR.PARAM_KEYS[1:]]                        # the library's order: branches, then heads
    mod.zero_grad(set_to_none=True)
    new_rays, weight, img_embed = _RigidBlurFn.apply(mod._desc(x.shape[1], 0), r, None, x, None, *net)
    ((new_rays * T(c["proj"]["new_rays"])).sum() + (weight * T(c["proj"]["weight"])).sum() + (img_embed * T(c["proj"]["img_embed"])).sum()).backward()
    assert np.array_equal(new_rays.detach().cpu().numpy(), out["new_rays"]) and np.array_equal(weight.detach().cpu().numpy(), out["weight"])
    assert torch.equal(img_embed.detach(), x.detach())
    for k, p in mod.named_parameters():
        if k != RR.PARAM_KEYS[0]:
            assert np.array_equal(p.grad.cpu().numpy(), grads[k]), k
    assert np.array_equal(r.grad.cpu().numpy(), d_rays)
    ref = RR.run(c["params"], c["rays"], None, c["M"], c["use_origin"], c["rv_window"], c["proj"]["new_rays"], c["proj"]["weight"],
                 c["proj"]["img_embed"], x=c["params"][RR.PARAM_KEYS[0]][c["ids"]])
    e = RR.rel_l2(x.grad.cpu().numpy(), ref["d_x"])
    print(f"per-ray form d x: {e:.2e} of the norm (bound {FACTOR:.0f} x {c['err_g'][RR.PARAM_KEYS[0]]:.2e})")
    assert e <= FACTOR * c["err_g"][RR.PARAM_KEYS[0]]
    summed = np.zeros_like(grads[RR.PARAM_KEYS[0]], dtype=np.float64)
    np.add.at(summed, c["ids"], x.grad.cpu().numpy().astype(np.float64))
    assert RR.rel_l2(grads[RR.PARAM_KEYS[0]], summed) < 1e-6                         # float32 sums of at most 34 rows


@pytest.mark.parametrize("R", [1, 15, 16, 17])
def test_tile_edges(R):
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, "regular")
    rays, ids, proj = _subset(c, np.arange(R) + 40)
    mod = _module(c)
    out, grads, d_rays = _run(mod, c, rays, ids, proj)
    ref = RR.run(c["params"], rays, ids, c["M"], c["use_origin"], c["rv_window"], proj["new_rays"], proj["weight"], proj["img_embed"])
    worst = max(c["err_g"].values())
    errs = {k: float(np.abs(out[k] - ref[k]).max()) for k in ("new_rays", "weight")}
    gerr = {k: RR.rel_l2(grads[k], ref["grads"][k]) for k in RR.PARAM_KEYS}
    gerr["rays"] = RR.rel_l2(d_rays, ref["d_rays"])
    print(f"R = {R}: outputs", {k: f"{v:.1e}" for k, v in errs.items()}, "gradients", {k: f"{v:.1e}" for k, v in gerr.items()}, f"bound {FACTOR:.0f} x {worst:.2e}")
    for k, e in errs.items():
        assert e <= FACTOR * c["err_out"][k], (k, e)
    assert max(gerr.values()) <= FACTOR * worst, gerr
    absent = sorted(set(range(c["params"][RR.PARAM_KEYS[0]].shape[0])) - set(ids.tolist()))
    assert not grads[RR.PARAM_KEYS[0]][absent].any()


def test_empty_batch_is_a_no_op():
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, "regular")
    mod = _module(c)
    rays, ids, proj = _subset(c, np.arange(0))
    out, grads, d_rays = _run(mod, c, rays, ids, proj)
    assert out["new_rays"].shape == (0, 10, 3, 2) and out["weight"].shape == (0, 10) and out["img_embed"].shape == (0, 32) and d_rays.shape == (0, 3, 2)
    assert all(not v.any() for v in grads.values())


def test_backward_twice_gives_the_same_bits_and_more_tiles_than_workgroups():
    """1100 rays = 69 tiles on at most 64 workgroups: some take two tiles with their weight-gradient accumulators resident"""
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, "regular")
    rs = np.random.RandomState(11)
    R = 1100
    idx = rs.randint(0, c["rays"].shape[0], R)
    rays = c["rays"][idx] + rs.uniform(-0.01, 0.01, (R, 3, 2)).astype(np.float32)
    ids = rs.choice([0, 1, 2, 4, 5, 6], R).astype(np.int64)
    proj = dict(new_rays=rs.standard_normal((R, 10, 3, 2)).astype(np.float32), weight=rs.standard_normal((R, 10)).astype(np.float32),
                img_embed=rs.standard_normal((R, 32)).astype(np.float32))
    mod = _module(c)
    out1, g1, d1 = _run(mod, c, rays, ids, proj)
    out2, g2, d2 = _run(mod, c, rays, ids, proj)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    assert np.array_equal(d1, d2) and all(np.array_equal(out1[k], out2[k]) for k in out1)
    ref = RR.run(c["params"], rays, ids, c["M"], c["use_origin"], c["rv_window"], proj["new_rays"], proj["weight"], proj["img_embed"])
    worst = max(c["err_g"].values())
    gerr = {k: RR.rel_l2(g1[k], ref["grads"][k]) for k in RR.PARAM_KEYS}
    gerr["rays"] = RR.rel_l2(d1, ref["d_rays"])
    errs = {k: float(np.abs(out1[k] - ref[k]).max()) for k in ("new_rays", "weight")}
    print("R = 1100: outputs", {k: f"{v:.1e}" for k, v in errs.items()}, "gradients", {k: f"{v:.1e}" for k, v in gerr.items()}, f"bound {FACTOR:.0f} x {worst:.2e}")
    for k, e in errs.items():
        assert e <= FACTOR * c["err_out"][k], (k, e)
    assert max(gerr.values()) <= FACTOR * worst, gerr
    assert not g1[RR.PARAM_KEYS[0]][RR.ABSENT_IMAGE].any()


def _widest():
    """-> module, its parameters, rays, ids, proj, M at the widest shape (test_widest_shape_against_float64)"""
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    rs = np.random.RandomState(37)
    C, Wd, M, R, n_img = 128, 64, 15, 17, 3
    mod = RigidBlurKernel(n_img, embed_dim=C, num_motion=M, W_r=Wd, W_v=Wd, W_w=Wd, use_origin=True, rv_window=0.1).to(DEV)
    assert {k for k, _ in mod.named_parameters()} == set(RR.PARAM_KEYS)
    params = {}
    for k, p in mod.named_parameters():
        scale = 1.0 if k == RR.PARAM_KEYS[0] else 0.5 if k.endswith("bias") else 1.0 / np.sqrt(p.shape[1])
        params[k] = (rs.standard_normal(tuple(p.shape)) * scale).astype(np.float32)
        with torch.no_grad():
            p.copy_(torch.tensor(params[k]))
    rays = rs.standard_normal((R, 3, 2)).astype(np.float32)
    ids = rs.choice([0, 2], R).astype(np.int64)                       # image 1 has no ray
    proj = dict(new_rays=rs.standard_normal((R, M + 1, 3, 2)).astype(np.float32), weight=rs.standard_normal((R, M + 1)).astype(np.float32),
                img_embed=rs.standard_normal((R, C)).astype(np.float32))
    return mod, params, rays, ids, proj, M


def test_widest_shape_against_float64():
    """The largest weight-gradient job table the kernel is built for (embed_dim 128, hidden widths 64, num_motion 15: 143 tiles), on two tiles
    of rays, the second holding one ray, with an image that has no ray.  Seeded normal table, rays and parameters (weights / sqrt(fan in),
    biases x 0.5, so the ReLU gates are mixed).  No fixture records the reference's float32 error here, so the bound is measured: the
    restatement in float32 against itself in float64 on the same inputs, times 4 for a different summation order; outputs get the floor
    2^-23 max|value|."""
    mod, params, rays, ids, proj, M = _widest()
    out1, g1, d1 = _run(mod, None, rays, ids, proj)
    out2, g2, d2 = _run(mod, None, rays, ids, proj)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    assert np.array_equal(d1, d2) and all(np.array_equal(out1[k], out2[k]) for k in out1)
    args = (params, rays, ids, M, True, 0.1, proj["new_rays"], proj["weight"], proj["img_embed"])
    ref, f32 = RR.run(*args), RR.run(*args, dtype=torch.float32)
    errs, bounds = {}, {}
    for k in ("new_rays", "weight"):
        errs[k] = float(np.abs(out1[k] - ref[k]).max())
        bounds[k] = max(FACTOR * float(np.abs(f32[k].astype(np.float64) - ref[k]).max()), 2.0 ** -23 * float(np.abs(ref[k]).max()))
    gerr = {k: RR.rel_l2(g1[k], ref["grads"][k]) for k in RR.PARAM_KEYS}
    gbound = {k: FACTOR * RR.rel_l2(f32["grads"][k], ref["grads"][k]) for k in RR.PARAM_KEYS}
    gerr["rays"], gbound["rays"] = RR.rel_l2(d1, ref["d_rays"]), FACTOR * RR.rel_l2(f32["d_rays"], ref["d_rays"])
    for k, e in errs.items():
        print(f"widest {k}: {e:.2e} (bound {bounds[k]:.2e})")
    for k, e in gerr.items():
        print(f"widest d {k}: {e:.2e} of the norm (bound {gbound[k]:.2e})")
    assert np.array_equal(out1["img_embed"], params[RR.PARAM_KEYS[0]][ids])
    assert not g1[RR.PARAM_KEYS[0]][1].any() and g1[RR.PARAM_KEYS[0]][[0, 2]].any(1).all()
    for k, e in errs.items():
        assert e <= bounds[k], (k, e, bounds[k])
    for k, e in gerr.items():
        assert e <= gbound[k], (k, e, gbound[k])


@pytest.mark.parametrize("kw,what", [(dict(D_r=2), "depth"), (dict(W_v=65), "width"), (dict(num_motion=16), "num_motion"), (dict(embed_dim=129), "feature")])
def test_rejected_shapes(kw, what):
    from evdeblurnerf_amd._lib import EvdError
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    mod = RigidBlurKernel(4, **kw).to(DEV)
    rays = torch.zeros((5, 3, 2), device=DEV)
    with pytest.raises(EvdError, match="evd_rigid_blur_forward") as ei:
        mod(400, 400, None, rays, {"images_idx": torch.zeros((5, 1), dtype=torch.int64, device=DEV)})
    assert what in str(ei.value)


def test_whole_training_call_with_the_real_kernel():
    """tests/test_gpu_train_call.py's G32 call with RigidBlurKernel (loaded with the state dict the reference's kernel had when G32 was
    recorded) where that file's stub replays recorded outputs"""
    from test_gpu_train_call import CALL_KW, G32_CASES, _model, rel
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    prec, awp_kind = "f16x3", "torch"
    tol = G32_CASES[(prec, awp_kind)]
    g = load_golden("G32_train_forward")
    g37 = load_golden("G37_rigid_blur")
    sd = {k[len("train_call.sd."):]: g37[k] for k in g37 if k.startswith("train_call.sd.")}
    kern = RigidBlurKernel.from_state_dict(sd, rv_window=0.1, use_origin=True).to(DEV)
    seen = {}
    kern.register_forward_hook(lambda m, i, o: seen.update(new_rays=o[0], weight=o[1], img_embed=o[3]["img_embed"]))
    model, awp, _ = _model(32, g, prec, awp_kind, kern)
    assert {k for k, _ in model.named_parameters() if k.startswith("kernelsnet.")} == {"kernelsnet." + k for k in RR.PARAM_KEYS}
    rays = torch.tensor(g["rays"], device=DEV)
    info = {"images_idx": torch.tensor(g["images_idx"], device=DEV)}
    rgb, rgb1, other_loss, other_tensors = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, rays_info=info, force_naive=False, return_pts0_rgb=True, **CALL_KW)
    out = dict(rgb=rgb, rgb1=rgb1, rgb_awp=other_tensors["rgb_awp"], stage1_rgb_pts0=other_tensors["stage1_rgb_pts0"], stage1_rgb1_pts0=other_tensors["stage1_rgb1_pts0"])
    e_rays = float(np.abs(seen["new_rays"].detach().cpu().numpy() - g["new_rays"]).max())
    e_w = float(np.abs(seen["weight"].detach().cpu().numpy() - g["weight"]).max())
    print(f"whole call: new_rays {e_rays:.2e} (bound {FACTOR * 5.1e-7:.2e}), weight {e_w:.2e} (bound {FACTOR * 1.9e-8:.2e})")
    assert np.array_equal(seen["img_embed"].detach().cpu().numpy(), g["img_embed"])
    assert torch.equal(other_tensors["stage1_img_embed"], seen["img_embed"])
    loss = sum((out[k] * torch.tensor(g["proj." + k], device=DEV)).sum() for k in out) + 0.1 * other_loss["TV"].sum()
    loss.backward()
    side = {k: rel(p.grad.cpu().numpy(), g["g.kernel." + k]) for k, p in kern.named_parameters()}
    print("whole call: kernel parameter gradients, error / norm:", {k: f"{v:.1e}" for k, v in side.items()}, f"(bound {tol['side']:.0e})")
    assert e_rays <= FACTOR * 5.1e-7 and e_w <= FACTOR * 1.9e-8
    assert abs(loss.item() - float(g["loss"])) < 200 * tol["out_all"]
    assert set(side) == set(RR.PARAM_KEYS) and max(side.values()) < tol["side"], side
