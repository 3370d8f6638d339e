"""ViewEmbeddingMLP on the device (csrc/kernel_view_embed.hip through evdeblurnerf_amd.blurmodel.ViewEmbeddingMLP.feature_table) against the
float64 restatement tests/view_embed_ref.py on golden G40's five cases, alone and as the table of RigidBlurKernel / SparseBlurKernel.

Bounds (tests/test_gpu_rigid_blur.py's rule).  The kernels get the REFERENCE's own float32 error as G40 records it (ref_f32_err: the real
module in float32 against itself in float64; max abs for outputs, relative L2 per gradient tensor), times 4 for a different summation
order.  Where a record is below the a-priori error of the computation itself, D (K_max + 1) 2^-24 with K_max the longest dot product
(view_embed_ref.floor), that floor stands in for the record: one gradient tensor of the case 'one' has the record 0.  For an output of a blur
kernel behind the table the floor is the rounding of the stored float32 value itself, 2^-24 of the largest value (DSK's align, a batch mean,
has records down to 9e-9).  A test on a subset
of a case's rows uses the case's worst tensor's record.  Every test prints what it observed beside its bound."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import rigid_blur_ref as RR
import sparse_blur_ref as SR
import view_embed_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0
KMAT = np.array([[350, 0, 200], [0, 350, 200], [0, 0, 1]], np.float32)


def T(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _case(tag):
    return VR.g40_case(load_golden("G40_view_embed_mlp"), tag)


def _mlp(params, skips):
    from evdeblurnerf_amd.blurmodel import ViewEmbeddingMLP
    n_img, E = params["img_embed"].shape
    mod = ViewEmbeddingMLP(VR.depth(params), params["view_embed_linears.0.weight"].shape[0], skips, n_img, E)
    mod.load_state_dict({k: torch.tensor(v) for k, v in params.items()}, strict=True)
    return mod.to(DEV)


def _alone(mod, ids, proj):
    """-> feature table, {name: gradient} of sum(table[ids] * proj)"""
    mod.zero_grad(set_to_none=True)
    table = mod.feature_table()
    (table[T(ids)] * T(proj)).sum().backward()
    return table.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in mod.named_parameters()}


def _bound(record, floor):
    return FACTOR * max(record, floor)


@pytest.mark.parametrize("tag", VR.G40_CASES)
def test_G40_table_and_gradients(tag):
    c = _case(tag)
    ref = VR.run(c["params"], c["skips"], c["ids"], c["proj"])
    floor = VR.floor(c["params"])
    table, grads = _alone(_mlp(c["params"], c["skips"]), c["ids"], c["proj"])
    assert table.shape == (c["n_img"], c["W"]) and set(grads) == set(VR.param_keys(c["D"]))
    e_t = float(np.abs(table - ref["table"]).max())
    gerr = {k: VR.rel_l2(grads[k], ref["grads"][k]) for k in grads}
    print(f"G40 {tag} table: {e_t:.2e} (bound {_bound(c['alone']['err_out']['table'], floor):.2e}; record {c['alone']['err_out']['table']:.2e}, floor {floor:.2e})")
    for k, e in gerr.items():
        print(f"G40 {tag} d {k}: {e:.2e} of the norm (bound {_bound(c['alone']['err_g'][k], floor):.2e}; record {c['alone']['err_g'][k]:.2e})")
    if c["absent"] is not None:
        assert not grads["img_embed"][c["absent"]].any()
        assert np.abs(grads["img_embed"]).sum(1).astype(bool).sum() == len(set(c["ids"].tolist()))
    assert e_t <= _bound(c["alone"]["err_out"]["table"], floor)
    for k, e in gerr.items():
        assert e <= _bound(c["alone"]["err_g"][k], floor), (k, e)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_tile_edges(n):
    """the first n rows of the case 'skip''s table (17 images) or 'shipped''s (34): tiles of 16 images with 1, 15, 16, 17 rows and two full ones + 1"""
    c = _case("skip" if n <= 17 else "shipped")
    params = dict(c["params"], img_embed=c["params"]["img_embed"][:n])
    rs = np.random.RandomState(n)
    ids = rs.choice([i for i in range(n) if n == 1 or i != n // 2], size=40).astype(np.int64)         # image n // 2 has no ray
    proj = rs.standard_normal((40, c["W"])).astype(np.float32)
    ref = VR.run(params, c["skips"], ids, proj)
    table, grads = _alone(_mlp(params, c["skips"]), ids, proj)
    floor = VR.floor(params)
    worst = max(c["alone"]["err_g"].values())
    e_t = float(np.abs(table - ref["table"]).max())
    gerr = {k: VR.rel_l2(grads[k], ref["grads"][k]) for k in grads}
    print(f"n_img = {n}: table {e_t:.1e} (bound {_bound(c['alone']['err_out']['table'], floor):.1e}), gradients", {k: f"{v:.1e}" for k, v in gerr.items()},
          f"(bound {_bound(worst, floor):.1e})")
    assert table.shape == (n, c["W"]) and e_t <= _bound(c["alone"]["err_out"]["table"], floor)
    assert max(gerr.values()) <= _bound(worst, floor), gerr
    if n > 1:
        assert not grads["img_embed"][n // 2].any()


@pytest.mark.parametrize("D,n,seed", [(4, 3, 818), (8, 19, 8)])
def test_widest_supported_networks(D, n, seed):
    """E = W = 128, every layer but the last a skip: the backward's weight-gradient tiles (480 at D = 4, 1024 at D = 8) spread over several
    workgroups per image tile, and its LDS rows pass 64 KiB.  No golden at these sizes: the bound is the a-priori error D (K_max + 1) 2^-24 (of
    the largest value for the table, of the norm for a gradient), times 4.  The D = 4 draw keeps every ReLU off the fence (asserted); no draw of
    the D = 8 network does (19 k units against a threshold of 2.5e-4), so there only the table, the absent image's row and the bits of a
    second run are checked."""
    rs = np.random.RandomState(seed)
    E = W = 128
    params = {"img_embed": rs.standard_normal((n, E)).astype(np.float32)}
    for i in range(D):
        fan = E if i == 0 else E + W
        params[f"view_embed_linears.{i}.weight"] = (rs.standard_normal((W, fan)) * (2.0 / fan) ** 0.5).astype(np.float32)
        params[f"view_embed_linears.{i}.bias"] = (0.1 * rs.standard_normal(W)).astype(np.float32)
    skips = list(range(D - 1))
    ids = rs.choice([i for i in range(n) if i != 1], size=40).astype(np.int64)
    proj = rs.standard_normal((40, W)).astype(np.float32)
    ref = VR.run(params, skips, ids, proj)
    mod = _mlp(params, skips)
    table, grads = _alone(mod, ids, proj)
    table2, grads2 = _alone(mod, ids, proj)
    bound = FACTOR * VR.floor(params)
    margin, thr = VR.fence_margin(params, skips)
    e_t = float(np.abs(table - ref["table"]).max() / np.abs(ref["table"]).max())
    gerr = {k: VR.rel_l2(grads[k], ref["grads"][k]) for k in grads}
    print(f"D = {D}: fence margin {margin:.1e} (threshold {thr:.1e}); table {e_t:.1e} of the largest value, gradients up to {max(gerr.values()):.1e} of the norm (bound {bound:.1e})")
    assert e_t <= bound and not grads["img_embed"][1].any()
    assert np.array_equal(table, table2) and all(np.array_equal(grads[k], grads2[k]) for k in grads)
    if D == 4:
        assert margin >= thr and max(gerr.values()) <= bound, gerr


def test_a_row_does_not_depend_on_its_position():
    c = _case("wide")
    perm = np.random.RandomState(3).permutation(c["n_img"])
    with torch.no_grad():
        a = _mlp(c["params"], c["skips"]).feature_table().cpu().numpy()
        b = _mlp(dict(c["params"], img_embed=c["params"]["img_embed"][perm]), c["skips"]).feature_table().cpu().numpy()
    assert a.any() and np.array_equal(b, a[perm])


def _prefixed(grads, prefix):
    return {prefix + k: v for k, v in grads.items()}


def _rigid(c):
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel
    M, use_origin = (int(v) for v in c["rigid"]["inputs"]["args"])
    sd = dict(c["rigid"]["sd"], **_prefixed(c["params"], "view_embed_module."))
    return RigidBlurKernel.from_state_dict(sd, rv_window=0.1, use_origin=bool(use_origin)).to(DEV), M, bool(use_origin)


def _rigid_run(mod, c, x_form):
    from evdeblurnerf_amd.blurmodel import _RigidBlurFn
    mod.zero_grad(set_to_none=True)
    proj, ids = c["rigid"]["proj"], T(c["ids"])
    r = T(c["rigid"]["inputs"]["rays"]).requires_grad_(True)
    if x_form:
        named = dict(mod.named_parameters())
        x = mod.view_embed_module.feature_table()[ids].contiguous()
        new_rays, weight, img_embed = _RigidBlurFn.apply(mod._desc(x.shape[1], 0), r, None, x, None, *[named[k] for k in RR.PARAM_KEYS[1:]])
    else:
        new_rays, weight, _, extras = mod(400, 400, None, r, {"images_idx": ids.reshape(-1, 1)}, return_img_embed=True)
        img_embed = extras["img_embed"]
    ((new_rays * T(proj["new_rays"])).sum() + (weight * T(proj["weight"])).sum() + (img_embed * T(proj["img_embed"])).sum()).backward()
    out = {k: v.detach().cpu().numpy() for k, v in dict(new_rays=new_rays, weight=weight, img_embed=img_embed).items()}
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in mod.named_parameters()}
    grads["rays"] = r.grad.cpu().numpy()
    return out, grads


def _check_composed(what, c, part, out, grads, ref, ref_grads, own_prefix):
    floor = VR.floor(c["params"])
    rec = c[part]
    errs = {k: float(np.abs(out[k] - ref[k]).max()) for k in rec["err_out"]}
    obound = {k: _bound(rec["err_out"][k], 2.0 ** -24 * float(np.abs(ref[k]).max())) for k in errs}       # (floor: the rounding of the stored value itself)
    gerr = {k: VR.rel_l2(grads[k], ref_grads[k]) for k in grads}
    for k, e in errs.items():
        print(f"{what} {k}: {e:.2e} (bound {obound[k]:.2e}; record {rec['err_out'][k]:.2e})")
    for k, e in gerr.items():
        print(f"{what} d {k}: {e:.2e} of the norm (bound {_bound(rec['err_g'][k], floor if k.startswith(own_prefix) else 0.0):.2e})")
    assert set(grads) == set(ref_grads) == set(rec["err_g"])
    for k, e in errs.items():
        assert e <= obound[k], (k, e)
    for k, e in gerr.items():
        assert e <= _bound(rec["err_g"][k], floor if k.startswith(own_prefix) else 0.0), (k, e)


@pytest.mark.parametrize("tag", VR.G40_CASES)
def test_as_the_table_of_the_rigid_blur_kernel(tag):
    c = _case(tag)
    mod, M, use_origin = _rigid(c)
    out, grads = _rigid_run(mod, c, False)
    with torch.no_grad():
        rows = mod.view_embed_module.feature_table()[T(c["ids"])].cpu().numpy()
    assert np.array_equal(out["img_embed"], rows)
    out_x, grads_x = _rigid_run(mod, c, True)                      # the existing per-ray form fed the gathered rows
    assert all(np.array_equal(out[k], out_x[k]) for k in out)
    assert all(np.array_equal(grads[k], grads_x[k]) for k in grads if not k.startswith("view_embed_module.")), "network tensors / d rays"
    table64 = VR.forward(c["params"], c["skips"])
    proj = c["rigid"]["proj"]
    ref = RR.run(dict({k: v for k, v in c["rigid"]["sd"].items()}, **{RR.PARAM_KEYS[0]: table64}), c["rigid"]["inputs"]["rays"], c["ids"], M, use_origin, 0.1,
                 proj["new_rays"], proj["weight"], proj["img_embed"])
    ref_grads = {k: v for k, v in ref["grads"].items() if k != RR.PARAM_KEYS[0]}
    ref_grads.update(_prefixed(VR.backward(c["params"], c["skips"], ref["grads"][RR.PARAM_KEYS[0]]), "view_embed_module."))
    ref_grads["rays"] = ref["d_rays"]
    _check_composed(f"G40 {tag} rigid", c, "rigid", out, grads, ref, ref_grads, "view_embed_module.")
    worst = max(c["rigid"]["err_g"].values())
    for k in grads_x:                                              # (the per-ray route sums an image's rows with atomics: tolerance, not bits)
        assert VR.rel_l2(grads_x[k], ref_grads[k]) <= _bound(worst, VR.floor(c["params"])), k
    if c["absent"] is not None:
        assert not grads["view_embed_module.img_embed"][c["absent"]].any()


def _sparse(c):
    from evdeblurnerf_amd.blurmodel import SparseBlurKernel
    sd = dict(c["dsk"]["sd"], **_prefixed(c["params"], "img_embed."))
    return SparseBlurKernel.from_state_dict(sd, "DSK", 10).to(DEV)


def _sparse_run(mod, c, x_form):
    from evdeblurnerf_amd.blurmodel import _SparseBlurFn
    mod.zero_grad(set_to_none=True)
    i, proj, ids = c["dsk"]["inputs"], c["dsk"]["proj"], T(c["ids"])
    if x_form:
        x = mod.img_embed.feature_table()[ids].contiguous()
        new_rays, weight, align, img_embed = _SparseBlurFn.apply(mod._desc(400, 400, KMAT, x.shape[1], 0), ids, x, T(i["rays_x"]).reshape(-1), T(i["rays_y"]).reshape(-1),
                                                                 T(i["poses"]), T(i["noise"]), None, mod.pattern_pos, None, None, *mod._net())
        align = align.reshape(())
    else:
        info = {"images_idx": ids.reshape(-1, 1), "rays_x": T(i["rays_x"]), "rays_y": T(i["rays_y"]), "poses": T(i["poses"])}
        new_rays, weight, align, extras = mod(400, 400, KMAT, None, info, return_img_embed=True, noise=T(i["noise"]))
        img_embed = extras["img_embed"]
    ((new_rays * T(proj["new_rays"])).sum() + (weight * T(proj["weight"])).sum() + (img_embed * T(proj["img_embed"])).sum() + SR.ALIGN_C * align).backward()
    out = {k: v.detach().cpu().numpy() for k, v in dict(new_rays=new_rays, weight=weight, img_embed=img_embed, align=align.reshape(1)).items()}
    return out, {k: p.grad.detach().cpu().numpy().copy() for k, p in mod.named_parameters()}


@pytest.mark.parametrize("tag", VR.G40_CASES)
def test_as_the_table_of_the_sparse_blur_kernel(tag):
    c = _case(tag)
    mod = _sparse(c)
    out, grads = _sparse_run(mod, c, False)
    with torch.no_grad():
        rows = mod.img_embed.feature_table()[T(c["ids"])].cpu().numpy()
    assert np.array_equal(out["img_embed"], rows)
    out_x, grads_x = _sparse_run(mod, c, True)
    assert all(np.array_equal(out[k], out_x[k]) for k in out)
    assert all(np.array_equal(grads[k], grads_x[k]) for k in grads if not k.startswith("img_embed.")), "network tensors"
    cfg = {k: (str(v) if k == "kernel_type" else float(v) if k == "random_hwindow" else int(v)) for k, v in c["dsk"]["cfg"].items()}
    i = c["dsk"]["inputs"]
    table64 = VR.forward(c["params"], c["skips"])
    ref = SR.run(dict(c["dsk"]["sd"], **{"img_embed.img_embed": table64}), cfg, 400, 400, tuple(float(v) for v in i["K4"]), c["ids"], i["rays_x"], i["rays_y"],
                 i["poses"], i["noise"], c["dsk"]["proj"])
    ref = dict(ref, align=np.asarray(ref["align"]).reshape(1))
    ref_grads = {k: v for k, v in ref["grads"].items() if k != "img_embed.img_embed"}
    ref_grads.update(_prefixed(VR.backward(c["params"], c["skips"], ref["grads"]["img_embed.img_embed"]), "img_embed."))
    _check_composed(f"G40 {tag} dsk", c, "dsk", out, grads, ref, ref_grads, "img_embed.")
    if c["absent"] is not None:
        assert not grads["img_embed.img_embed"][c["absent"]].any()


def test_two_runs_give_the_same_bits():
    c = _case("skip")
    mod = _mlp(c["params"], c["skips"])
    t1, g1 = _alone(mod, c["ids"], c["proj"])
    t2, g2 = _alone(mod, c["ids"], c["proj"])
    assert np.array_equal(t1, t2) and all(np.array_equal(g1[k], g2[k]) for k in g1)
    rk, _, _ = _rigid(c)
    sk = _sparse(c)
    for run, m in ((_rigid_run, rk), (_sparse_run, sk)):
        o1, g1 = run(m, c, False)
        o2, g2 = run(m, c, False)
        assert all(np.array_equal(o1[k], o2[k]) for k in o1) and all(np.array_equal(g1[k], g2[k]) for k in g1)
        assert all(np.isfinite(v).all() and v.any() for v in g1.values())


@pytest.mark.parametrize("kernel_type", ["RBK", "DSK"])
def test_training_iteration_through_NeRFAll(kernel_type):
    """tests/test_gpu_train_call.py's toy c2f model (5 points per pixel, AWP on a feature of width 32) with a from_args(param_mlp) kernel: one
    forward in training mode, backward, dist.GradReducer and optim.Adam with no special case"""
    from types import SimpleNamespace
    from test_gpu_train_call import CALL_KW, _model
    from test_view_embed_module import _args
    from evdeblurnerf_amd import dist as D, optim as O, weights as W
    from evdeblurnerf_amd.blurmodel import RigidBlurKernel, SparseBlurKernel
    g = load_golden("G32_train_forward")
    R, n_imgs = 32, 6
    torch.manual_seed(40)
    args = _args(kernel_img_embed=24, kernel_img_mlp_embed=32, kernel_img_mlp_depth=3, kernel_img_mlp_skips=0, kernel_type=kernel_type, kernel_num_wide=32,
                 kernel_num_hidden=2)
    kern = (RigidBlurKernel if kernel_type == "RBK" else SparseBlurKernel).from_args(args, n_imgs).to(DEV)
    model, awp, _ = _model(32, g, "f16x3", "torch", kern)
    model.kernel_type = kernel_type
    rs = np.random.RandomState(6)
    ids = rs.randint(0, n_imgs - 1, (R, 1))                                            # the last image has no ray
    info = {"images_idx": T(ids.astype(np.int64))}
    kw = {}
    if kernel_type == "DSK":
        poses = np.concatenate([np.eye(3, dtype=np.float32)[None].repeat(R, 0), 0.1 * rs.standard_normal((R, 3, 1)).astype(np.float32)], -1)
        info.update(rays_x=T(rs.randint(0, 400, (R, 1)).astype(np.float32)), rays_y=T(rs.randint(0, 400, (R, 1)).astype(np.float32)), poses=T(poses))
        kw["kernel_noise"] = T(rs.standard_normal((R, 5, 2)).astype(np.float32))
    rays = T(g["rays"][:R])
    rgb, rgb1, other_loss, other_tensors = model(400, 400, W.synthetic_camera(), 1 << 20, rays=rays, rays_info=info, force_naive=False, return_pts0_rgb=True,
                                                 **kw, **CALL_KW)
    proj = {k: T(rs.standard_normal((R, 3)).astype(np.float32)) for k in ("rgb", "rgb1", "rgb_awp")}
    loss = (rgb * proj["rgb"]).sum() + (rgb1 * proj["rgb1"]).sum() + (other_tensors["rgb_awp"] * proj["rgb_awp"]).sum() + 0.1 * other_loss["TV"].sum()
    if "align" in other_loss:
        loss = loss + 0.3 * other_loss["align"].sum()
    loss.backward()
    red = D.GradReducer(list(model.parameters()))
    red.start()
    red.wait()
    own = {k: p for k, p in model.named_parameters() if "view_embed_linears." in k or k.endswith(".img_embed")}
    assert len(own) == 1 + 2 * 3 and all(k.startswith("kernelsnet.") for k in own)
    for k, p in own.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.any(), k
    embed = [p for k, p in own.items() if k.endswith(".img_embed")][0]
    assert not embed.grad[n_imgs - 1].any() and embed.grad[:n_imgs - 1].abs().sum(1).bool().all()
    before = {k: p.detach().clone() for k, p in own.items()}
    O.Adam(model.parameters(), lr=1e-3, model=model).step()
    for k, p in own.items():
        assert not torch.equal(p.detach(), before[k]), k
