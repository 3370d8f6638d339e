"""Pins the reference of tests/test_gpu_ray_frontend.py (tests/ray_ref.py over tests/fe_bound.py) before any kernel is held to it.  CPU only.

  * the float32 numpy instantiation of every function -- the stand-in for a correct kernel -- lies inside the Fe bound at a factor of 1,
    on every element of the inputs the GPU file uses (and no divisor of those inputs comes near 0: Fe asserts |b| > 2 eb);
  * the Fe values agree with the CPU oracle and with the reference's goldens G1, G6, G16 and the nohalf_* part of G28, within the bound;
  * the closed form of k_ray_batch_bwd equals float64 autograd of the forward restatement to 1e-12;
  * ten planted faults, applied to the stand-in, leave the bound (the ratios are printed);
  * through the C ABI with dummy pointers (a valid call is never made): the front end's entries refuse a null input with a positive count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fe_bound as fb
import ray_ref as rr
from conftest import load_golden
from fe_bound import Fe
from oracle import oracle as O

LIFT, F32 = Fe.lift, rr.f32


def inside(tag, got, fe, report):
    q, where = fb.ratio(got, fe)
    report[tag] = max(report.get(tag, 0.0), q)
    assert q <= 1.0, (tag, q, where)


@pytest.fixture(scope="module")
def report():
    r = {}
    yield r
    for k, v in r.items():
        print(f"ray_ref {k}: worst error / bound = {v:.3f}")


# ------------------------------------------------------------------------------------------------ the stand-in inside the bound
def test_standin_camera(report):
    for c in rr.cases_get_rays():
        for tag, a, b in zip("od", rr.get_rays_arrays(LIFT, **c), rr.get_rays_arrays(F32, **c)):
            inside("get_rays." + tag, b, a, report)
    for c in rr.cases_get_rays_pix():
        for tag, a, b in zip("od", rr.get_rays_pix_arrays(LIFT, **c), rr.get_rays_pix_arrays(F32, **c)):
            inside("get_rays_pix." + tag, b, a, report)


def test_standin_ndc_and_ray_batch(report):
    for c in rr.cases_ndc():
        for tag, a, b in zip("od", rr.ndc_arrays(LIFT, **c), rr.ndc_arrays(F32, **c)):
            inside("ndc." + tag, b, a, report)
    for c in rr.cases_ray_batch():
        a, b = rr.ray_batch_arrays(LIFT, **c), rr.ray_batch_arrays(F32, **c)
        assert b.shape == (len(c["rays"]), 11 if c["use_viewdirs"] else 8) and b.dtype == np.float32
        inside("ray_batch", b, a, report)


def test_standin_rbk_warp(report):
    for c, _ in rr.cases_rbk():
        for tag, a, b in zip(("rays", "T"), rr.rbk_warp_arrays(LIFT, **c), rr.rbk_warp_arrays(F32, **c)):
            inside("rbk_warp." + tag, b, a, report)
        P = c["M"] + c["use_origin"]
        assert b.shape == (len(c["rays"]), P, 4, 4)


def test_standin_embed(report):
    for c in rr.cases_embed():
        inside("embed", rr.embed_arrays(F32, **c), rr.embed_arrays(LIFT, **c), report)


def test_standin_backward_and_points(report):
    for c in rr.cases_ray_batch_bwd():
        inside("ray_batch_bwd", rr.ray_batch_bwd_arrays(F32, **c), rr.ray_batch_bwd_arrays(LIFT, **c), report)
    for c in rr.cases_points():
        inside("points", rr.points_arrays(F32, c["rb"], c["z"]), rr.points_arrays(LIFT, c["rb"], c["z"]), report)
        val, bound = rr.points_bwd_ref(c["z"], c["g"])
        inside("points_bwd", rr.points_bwd_f32(c["z"], c["g"]), Fe(val, bound), report)
        once = rr.points_bwd_f32(c["z"], c["g"], c["prev"][:, :6])
        inside("points_bwd.acc", once, Fe(*rr.points_bwd_ref(c["z"], c["g"], c["prev"][:, :6])), report)
        inside("points_bwd.acc", rr.points_bwd_f32(c["z"], c["g"], once), Fe(*rr.points_bwd_ref(c["z"], c["g"], once)), report)


# ------------------------------------------------------------------------------------------------ against the oracle and the goldens
def test_values_match_the_oracle(report):
    for c in rr.cases_get_rays():
        o, d = O.get_rays(c["H"], c["W"], c["K"], c["c2w"], c["add_halfpix"])
        fo, fd = rr.get_rays_arrays(LIFT, **c)
        inside("oracle.get_rays", o.reshape(-1, 3), fo, report)
        inside("oracle.get_rays", d.reshape(-1, 3), fd, report)
    for c in rr.cases_get_rays_pix():
        for got, fe in zip(O.get_rays_pix(c["coords"], c["K"], c["c2ws"], c["add_halfpix"]), rr.get_rays_pix_arrays(LIFT, **c)):
            inside("oracle.get_rays_pix", got, fe, report)
    for c in rr.cases_ndc():
        for got, fe in zip(O.ndc_rays(c["H"], c["W"], c["focal"], c["near"], c["o"], c["d"]), rr.ndc_arrays(LIFT, **c)):
            inside("oracle.ndc_rays", got, fe, report)
    for c in rr.cases_ray_batch():
        cfg = O.make_cfg(H=c["H"], W=c["W"], focal=c["focal"], ndc=c["ndc_on"], use_viewdirs=c["use_viewdirs"], near=c["near"], far=c["far"])
        inside("oracle.ray_batch", O.ray_batch(cfg, c["rays"]), rr.ray_batch_arrays(LIFT, **c), report)
    for c, _ in rr.cases_rbk():
        got = O.rbk_warp(c["rays"], c["r"], c["v"], c["M"], bool(c["use_origin"]), want_transform=True)
        for g, fe in zip(got, rr.rbk_warp_arrays(LIFT, **c)):
            inside("oracle.rbk_warp", g, fe, report)
    for c in rr.cases_embed():
        if c["L"] > 0:
            inside("oracle.embed", O.embed(c["x"], c["L"]), rr.embed_arrays(LIFT, **c), report)


def test_values_match_the_goldens(report):
    g = load_golden("G1_embedder")
    for L, key in ((10, "pe10"), (4, "pe4"), (2, "pe2")):
        inside("golden.G1", g[key], rr.embed_arrays(LIFT, g["x"], L), report)
    g = load_golden("G6_rays")
    fo, fd = rr.get_rays_arrays(LIFT, 60, 80, g["Kn"], g["c2w"])
    inside("golden.G6", g["rays_o_full"], fo.reshape(60, 80, 3)[::7, ::5], report)
    inside("golden.G6", g["rays_d_full"], fd.reshape(60, 80, 3)[::7, ::5], report)
    from evdeblurnerf_amd import weights as W
    K = W.synthetic_camera()
    for got, fe in zip((g["rays_o_pix"], g["rays_d_pix"]), rr.get_rays_pix_arrays(LIFT, g["coords"], K, g["poses"])):
        inside("golden.G6", got, fe, report)
    for got, fe in zip((g["ndc_o"], g["ndc_d"]), rr.ndc_arrays(LIFT, 400, 400, float(K[0, 0]), 1.0, g["rays_o_pix"], g["rays_d_pix"])):
        inside("golden.G6", got, fe, report)
    g = load_golden("G16_rbk_warp")
    for tag, M, uo in (("a", 9, 1), ("b", 4, 0), ("c", 9, 1)):
        nr, tf = rr.rbk_warp_arrays(LIFT, g[f"{tag}_rays"], g[f"{tag}_r"], g[f"{tag}_v"], M, uo)
        inside("golden.G16", g[f"{tag}_new_rays"], nr, report)
        inside("golden.G16", g[f"{tag}_transform"], tf, report)
    g = load_golden("G28_image_batch")
    for got, fe in zip((g["nohalf_pix_o"], g["nohalf_pix_d"]), rr.get_rays_pix_arrays(LIFT, g["nohalf_coords"], g["K"], g["nohalf_c2ws"], False)):
        inside("golden.G28", got, fe, report)
    H, Wd = g["images"].shape[1:3]
    fo, fd = rr.get_rays_arrays(LIFT, H, Wd, g["K"], g["poses"][1], False)
    inside("golden.G28", g["nohalf_full_o"].reshape(-1, 3), fo, report)
    inside("golden.G28", g["nohalf_full_d"].reshape(-1, 3), fd, report)


# ------------------------------------------------------------------------------------------------ the closed form against autograd
def autograd_ray_batch_bwd(H, W, focal, rays, g, ndc_on):
    """float64 autograd of the forward restatement, contracted with g (columns 6, 7 carry nothing)"""
    cw, ch = rr.ndc_coeffs(H, W, focal)
    r = torch.tensor(np.asarray(rays, np.float64), requires_grad=True)
    o, d, vd = rr.ray_batch(rr.cols(r[..., 0]), rr.cols(r[..., 1]), cw, ch, ndc_on, True)
    g = torch.tensor(np.asarray(g, np.float64))
    sum((x * g[:, k]).sum() for k, x in zip((0, 1, 2, 3, 4, 5, 8, 9, 10), o + d + vd)).backward()
    return r.grad.numpy()


def test_closed_form_backward_equals_autograd():
    worst = 0.0
    for c in rr.cases_ray_batch_bwd():
        fe = rr.ray_batch_bwd_arrays(LIFT, **c)
        auto = autograd_ray_batch_bwd(**c)
        # relative to the element where it is well conditioned, to the magnitude of its terms (err / u) where they cancel
        scale = np.maximum(np.abs(auto), 1e-3 * fe.err / fb.U)
        q = np.abs(fe.value - auto) / np.where(scale > 0, scale, 1.0)
        assert np.all((scale > 0) | (fe.value == auto))
        worst = max(worst, float(q.max()))
        assert q.max() <= 1e-12, (q.max(), np.unravel_index(q.argmax(), q.shape))
    print(f"closed form vs float64 autograd: worst relative difference {worst:.2e}")


# ------------------------------------------------------------------------------------------------ planted faults
def test_planted_faults_leave_the_bound():
    H, W, focal = rr.NDC_HWF
    cw, ch = rr.ndc_coeffs(H, W, focal)
    rs = np.random.RandomState(5)
    rays = rr.make_rays(rs, 257)
    o, d = rays[..., 0], rays[..., 1]
    out = {}

    fe = fb.stack(sum(rr.ndc(cw, ch, 1.0, rr.cols(LIFT(o)), rr.cols(LIFT(d))), []))
    out["cw / ch swapped"] = fb.ratio(fb.stack(sum(rr.ndc(ch, cw, 1.0, rr.cols(F32(o)), rr.cols(F32(d))), [])), fe)[0]

    Hh, Ww, pose = 17, 300, rr.make_pose(rs)
    fe = rr.get_rays_arrays(LIFT, Hh, Ww, rr.K_TEST, pose)[1]
    x, y = rr.pixel_grid(Hh, Ww)
    idx = np.arange(Hh * Ww)
    Kn = [F32(rr.K_TEST[0, 0]), F32(rr.K_TEST[0, 2]), F32(rr.K_TEST[1, 1]), F32(rr.K_TEST[1, 2])]
    bad = rr.camera_rays(F32(idx // Ww), F32(idx % Ww), Kn, [F32(v) for v in pose.reshape(-1)])[1]
    out["pixel row / column transposed"] = fb.ratio(fb.stack(bad), fe)[0]
    out["half pixel dropped"] = fb.ratio(rr.get_rays_arrays(F32, Hh, Ww, rr.K_TEST, pose, False)[1], fe)[0]

    kw = dict(H=H, W=W, focal=focal, rays=rays, ndc_on=1, use_viewdirs=1, near=0.0, far=1.0)
    out["near = 2 in ray_batch's NDC call"] = fb.ratio(rr.ray_batch_arrays(F32, ndc_near=2.0, **kw), rr.ray_batch_arrays(LIFT, **kw))[0]

    g = rs.standard_normal((257, 11)).astype(np.float32)
    fe = rr.ray_batch_bwd_arrays(LIFT, H, W, focal, rays, g, 1)
    out["g_t (1 + o_z) / d_z^2 dropped from gd[2]"] = fb.ratio(rr.ray_batch_bwd_arrays(F32, H, W, focal, rays, g, 1, drop=("gt_dz2",)), fe)[0]
    out["view-direction projection dropped"] = fb.ratio(rr.ray_batch_bwd_arrays(F32, H, W, focal, rays, g, 1, drop=("proj",)), fe)[0]

    x = rs.uniform(-1.5, 1.5, (86, 3)).astype(np.float32)
    out["sin / cos swapped"] = fb.ratio(rr.embed_arrays(F32, x, 4, swap=True), rr.embed_arrays(LIFT, x, 4))[0]

    ry, r, v, _ = rr.make_rbk(rs, 29, 9)
    wrong = lambda a, M: [a.reshape(a.shape[0], M, 3)[:, :, c] for c in range(3)]
    out["r read as [R, M, 3]"] = fb.ratio(rr.rbk_warp_arrays(F32, ry, r, v, 9, 1, split=wrong)[0], rr.rbk_warp_arrays(LIFT, ry, r, v, 9, 1)[0])[0]

    c = next(k for k in rr.cases_points() if k["z"].shape == (5, 65))
    prev = c["prev"][:, :6]
    out["= for += when accumulating"] = fb.ratio(rr.points_bwd_f32(c["z"], c["g"], prev, assign=True), Fe(*rr.points_bwd_ref(c["z"], c["g"], prev)))[0]
    out["one butterfly step missing"] = fb.ratio(rr.points_bwd_f32(c["z"], c["g"], steps=(32, 16, 8, 4, 2)), Fe(*rr.points_bwd_ref(c["z"], c["g"])))[0]

    for k, q in out.items():
        print(f"planted fault: {k}: worst error / bound = {q:.3g}")
    assert len(out) == 10
    for k, q in out.items():
        assert q > 1.0, (k, q)


# ------------------------------------------------------------------------------------------------ argument checks through the C ABI
@pytest.fixture(scope="module")
def lib():
    from evdeblurnerf_amd import build, _lib
    build.build()
    return _lib.lib()


def P(on=1):
    """a dummy pointer (non-null = 0x1000): a valid call is never made here"""
    return C.c_void_p(0x1000) if on else None


def FP(on=1):
    return C.cast(C.c_void_p(0x1000), C.POINTER(C.c_float)) if on else None


def cfg(use_viewdirs=1):
    from evdeblurnerf_amd import _lib
    c = _lib.RenderCfg()
    c.H, c.W, c.focal, c.ndc, c.use_viewdirs, c.near, c.far = 300, 400, 350.0, 1, use_viewdirs, 0.0, 1.0
    return C.byref(c)


def refused(lib, rc, entry):
    assert rc == -1, (entry, rc)
    assert entry.encode() in lib.evd_last_error(), (entry, lib.evd_last_error())


def test_null_inputs_with_a_positive_count_are_refused(lib):
    for coords, c2ws in ((0, 1), (1, 0), (0, 0)):
        refused(lib, lib.evd_get_rays_pix(P(coords), FP(), P(c2ws), 5, 1, P(), P(), None), "evd_get_rays_pix")
    for o, d in ((0, 1), (1, 0), (0, 0)):
        refused(lib, lib.evd_ndc_rays(300, 400, 350.0, 1.0, P(o), P(d), 5, P(), P(), None), "evd_ndc_rays")
    refused(lib, lib.evd_embed(None, 5, 3, 4, P(), None), "evd_embed")
    for uv in (1, 0):
        refused(lib, lib.evd_ray_batch(cfg(uv), None, 5, P(), None), "evd_ray_batch")


def test_null_outputs_and_the_guarded_entries_stay_refused(lib):
    refused(lib, lib.evd_get_rays_pix(P(), FP(), P(), 5, 1, None, P(), None), "evd_get_rays_pix")
    refused(lib, lib.evd_get_rays_pix(P(), None, P(), 5, 1, P(), P(), None), "evd_get_rays_pix")
    refused(lib, lib.evd_ndc_rays(300, 400, 350.0, 1.0, P(), P(), 5, None, P(), None), "evd_ndc_rays")
    refused(lib, lib.evd_embed(P(), 5, 3, 4, None, None), "evd_embed")
    refused(lib, lib.evd_embed(P(), 5, 0, 4, P(), None), "evd_embed")
    refused(lib, lib.evd_ray_batch(cfg(), P(), 5, None, None), "evd_ray_batch")
    refused(lib, lib.evd_ray_batch(None, P(), 5, P(), None), "evd_ray_batch")
    for K, c2w, o, d in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        refused(lib, lib.evd_get_rays(4, 5, FP(K), FP(c2w), 1, P(o), P(d), None), "evd_get_rays")
    refused(lib, lib.evd_get_rays(0, 5, FP(), FP(), 1, P(), P(), None), "evd_get_rays")
    for rays, r, v, out in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        refused(lib, lib.evd_rbk_warp(P(rays), P(r), P(v), 5, 9, 1, P(out), None, None), "evd_rbk_warp")
    refused(lib, lib.evd_rbk_warp(P(), P(), P(), 5, 0, 1, P(), None, None), "evd_rbk_warp")
    for rays, g, out in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        refused(lib, lib.evd_ray_batch_bwd(cfg(), P(rays), P(g), 5, P(out), None), "evd_ray_batch_bwd")
    refused(lib, lib.evd_ray_batch_bwd(cfg(0), P(), P(), 5, P(), None), "evd_ray_batch_bwd")            # the 8-column batch has no backward
    for z, g, out in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        for acc in (0, 1):
            refused(lib, lib.evd_points_bwd(P(z), P(g), 5, 8, acc, P(out), None), "evd_points_bwd")
    refused(lib, lib.evd_points_bwd(P(), P(), 5, 0, 0, P(), None), "evd_points_bwd")


def test_a_count_of_zero_with_null_inputs_is_a_no_op(lib):
    assert lib.evd_get_rays_pix(None, FP(), None, 0, 1, P(), P(), None) == 0
    assert lib.evd_ndc_rays(300, 400, 350.0, 1.0, None, None, 0, P(), P(), None) == 0
    assert lib.evd_embed(None, 0, 3, 4, P(), None) == 0
    assert lib.evd_ray_batch(cfg(), None, 0, P(), None) == 0
    assert lib.evd_rbk_warp(None, None, None, 0, 9, 1, None, None, None) == 0
    assert lib.evd_ray_batch_bwd(cfg(), P(), P(), 0, P(), None) == 0
    assert lib.evd_points_bwd(P(), P(), 0, 8, 0, P(), None) == 0
