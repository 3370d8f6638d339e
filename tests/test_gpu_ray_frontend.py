"""The ray front end on the device against float64 with running error bounds: k_get_rays, k_get_rays_pix, k_ndc, k_ray_batch (8 and 11
columns), k_rbk_warp, k_embed, k_points and the hand-derived backward kernels k_ray_batch_bwd and k_points_bwd, each through its C entry.

These kernels run the reference's float32 operations one rounding at a time (no contraction, IEEE division and square root), so
tests/fe_bound.py bounds every element's distance from the exact value rigorously and the device has to stay inside that bound at a
factor of 1: |device - Fe.value| <= Fe.err for EVERY element.  tests/test_ray_ref.py pins the reference first (stand-in inside the bound,
oracle, goldens, float64 autograd, ten planted faults that leave the bound by 1e4 .. 2e7).  Where a kernel only copies (origins, near /
far, the use_origin slot with its identity transform, the identity block of the encoding) the bits are compared.  Outputs go into
NaN-filled buffers with 16 guard floats behind them: every element is written and the guard is not.  Each test prints the worst
error / bound and how many elements are not the bits of the float32 numpy stand-in (reported, not asserted).

Recorded figures (one MI355X).  Worst error / bound: get_rays 0.67, get_rays_pix 0.79, ndc_rays 0.56, ray_batch 0.61, rbk_warp 0.95 (new
rays) / 0.58 (transforms), embed 0.56, ray_batch_bwd 0.90, points 0.99, points_bwd 0.14 (overwrite) / 0.19 (accumulate).  The device gives
the float32 numpy stand-in's bits in every element of every kernel except where sinf / cosf enter (embed: 15659 of 93568 elements,
rbk_warp: 5132 of 37884 and 11788 of 101024): k_embed's sinf / cosf are within 1.12 u of float64, so K_TRIG stays at the 2 u of
tests/fe_bound.py and the torch-on-the-GPU yardstick was not needed (measured anyway on x 2^k, |x| <= 40, k < 10: 1.17 u, torch on the
CPU 0.60 u).  The bound on a warped ray's element by angle class (|v| up to 1), with the device's worst error / bound: |r| = 0: 1.1e-6
(0.95), 1e-6: 0.36 (0.00), 1e-3: 3.7e-4 (0.27), 1e-2: 4.1e-5 (0.31), 0.3: 7.6e-6 (0.37), 3.1: 2.5e-5 (0.17), 6.5: 1.6e-5 (0.21) -- what
an absolute K_TRIG u on 1 - cos and theta - sin, times v / theta, allows at small angles; the reference's formula loses the same.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fe_bound as fb
import ray_ref as rr
from fe_bound import Fe

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 16
LIFT, F32 = Fe.lift, rr.f32
_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def L():
    from evdeblurnerf_amd import _lib
    _lib.lib()
    return _lib


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_fp)


class Out:
    """a NaN-filled device buffer of n floats with GUARD more behind them"""

    def __init__(self, *shape, fill=None):
        self.shape = shape
        self.n = int(np.prod(shape))
        self.t = torch.full((self.n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        if fill is not None:
            self.t[:self.n] = T(fill).reshape(-1)

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def get(self, written=True):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert np.all(np.isnan(h[self.n:])), "the guard behind the output was written"
        out = h[:self.n].reshape(self.shape)
        if written:
            assert not np.any(np.isnan(out)), "an output element was not written"
        return out


def ok(L, rc, what):
    L.check(rc, what)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


class Report:
    def __init__(self, name):
        self.name, self.worst, self.differ, self.count = name, 0.0, 0, 0

    def inside(self, got, fe, standin=None, what=""):
        q, where = fb.ratio(got, fe)
        self.worst = max(self.worst, q)
        self.count += got.size
        if standin is not None:
            self.differ += int((np.asarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(standin, dtype=np.float32).view(np.uint32)).sum())
        assert q <= 1.0, (self.name, what, q, where)

    def done(self):
        print(f"{self.name}: worst error / bound = {self.worst:.3f}; {self.differ} of {self.count} elements are not the stand-in's bits")


def rcfg(L, H, W, focal, ndc_on, use_viewdirs, near=0.0, far=1.0):
    c = L.RenderCfg()
    c.H, c.W, c.focal, c.ndc, c.use_viewdirs, c.near, c.far = H, W, float(focal), int(ndc_on), int(use_viewdirs), near, far
    return c


# ------------------------------------------------------------------------------------------------ camera model
def test_get_rays(L):
    rep = Report("get_rays")
    for c in rr.cases_get_rays():
        H, W = c["H"], c["W"]
        (_, K), (pose, c2w) = host(c["K"]), host(c["c2w"])
        o, d = Out(H * W, 3), Out(H * W, 3)
        ok(L, L.lib().evd_get_rays(H, W, K, c2w, int(c["add_halfpix"]), o.ptr(), d.ptr(), L.stream_ptr()), "evd_get_rays")
        assert same_bits(o.get(), np.broadcast_to(pose[:, 3], (H * W, 3)))
        rep.inside(d.get(), rr.get_rays_arrays(LIFT, **c)[1], rr.get_rays_arrays(F32, **c)[1], (H, W, c["add_halfpix"]))
    rep.done()


def test_get_rays_pix(L):
    rep = Report("get_rays_pix")
    for c in rr.cases_get_rays_pix():
        n = len(c["coords"])
        _, K = host(c["K"])
        coords, c2ws = T(c["coords"]), T(c["c2ws"])
        o, d = Out(n, 3), Out(n, 3)
        ok(L, L.lib().evd_get_rays_pix(L.ptr(coords), K, L.ptr(c2ws), n, int(c["add_halfpix"]), o.ptr(), d.ptr(), L.stream_ptr()), "evd_get_rays_pix")
        assert same_bits(o.get(), c["c2ws"][:, :, 3])
        rep.inside(d.get(), rr.get_rays_pix_arrays(LIFT, **c)[1], rr.get_rays_pix_arrays(F32, **c)[1], (n, c["add_halfpix"]))
    rep.done()


# ------------------------------------------------------------------------------------------------ NDC warp, ray packing
def test_ndc_rays(L):
    rep = Report("ndc_rays")
    for c in rr.cases_ndc():
        n = len(c["o"])
        o, d = T(c["o"]), T(c["d"])
        oo, od = Out(n, 3), Out(n, 3)
        ok(L, L.lib().evd_ndc_rays(c["H"], c["W"], c["focal"], c["near"], L.ptr(o), L.ptr(d), n, oo.ptr(), od.ptr(), L.stream_ptr()), "evd_ndc_rays")
        for got, fe, st in zip((oo.get(), od.get()), rr.ndc_arrays(LIFT, **c), rr.ndc_arrays(F32, **c)):
            rep.inside(got, fe, st, (n, c["near"]))
    rep.done()


def test_ray_batch(L):
    rep = Report("ray_batch")
    for c in rr.cases_ray_batch():
        R, nc = len(c["rays"]), 11 if c["use_viewdirs"] else 8
        cfg = rcfg(L, c["H"], c["W"], c["focal"], c["ndc_on"], c["use_viewdirs"], c["near"], c["far"])
        rays, rb = T(c["rays"]), Out(R, nc)
        ok(L, L.lib().evd_ray_batch(C.byref(cfg), L.ptr(rays), R, rb.ptr(), L.stream_ptr()), "evd_ray_batch")
        got = rb.get()
        assert same_bits(got[:, 6:8], np.broadcast_to(np.float32([c["near"], c["far"]]), (R, 2)))
        if not c["ndc_on"]:
            assert same_bits(got[:, 0:3], c["rays"][..., 0]) and same_bits(got[:, 3:6], c["rays"][..., 1])
        rep.inside(got, rr.ray_batch_arrays(LIFT, **c), rr.ray_batch_arrays(F32, **c), (R, nc, c["ndc_on"]))
    rep.done()


# ------------------------------------------------------------------------------------------------ SE(3) exponential of the blur kernel
def test_rbk_warp(L):
    rep_r, rep_t = Report("rbk_warp new_rays"), Report("rbk_warp transforms")
    per_class = {}
    for c, cls in rr.cases_rbk():
        R, M, uo = len(c["rays"]), c["M"], c["use_origin"]
        P = M + uo
        rays, r, v = T(c["rays"]), T(c["r"]), T(c["v"])
        fe_r, fe_t = rr.rbk_warp_arrays(LIFT, **c)
        st_r, st_t = rr.rbk_warp_arrays(F32, **c)
        outs = []
        for with_tf in (1, 0):
            nr, tf = Out(R, P, 3, 2), Out(R, P, 4, 4)
            ok(L, L.lib().evd_rbk_warp(L.ptr(rays), L.ptr(r), L.ptr(v), R, M, uo, nr.ptr(), tf.ptr() if with_tf else None, L.stream_ptr()), "evd_rbk_warp")
            outs.append(nr.get())
            got_t = tf.get(written=bool(with_tf))
            if with_tf:
                rep_r.inside(outs[0], fe_r, st_r, (R, M, uo))
                rep_t.inside(got_t, fe_t, st_t, (R, M, uo))
                assert same_bits(got_t[:, :, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), (R, P, 4)))
                if uo:
                    assert same_bits(outs[0][:, 0], c["rays"])
                    assert same_bits(got_t[:, 0], np.broadcast_to(np.eye(4, dtype=np.float32), (R, 4, 4)))
            else:
                assert np.all(np.isnan(got_t))                   # a null `transforms` writes none
        assert same_bits(outs[0], outs[1])
        for k in range(len(rr.RBK_NORMS)):
            m = cls == k
            if m.any():
                q = fb.ratio(outs[0][m][:, uo:], fe_r[m][:, uo:])[0]
                e = float(fe_r.err[m][:, uo:].max())
                a, b = per_class.get(k, (0.0, 0.0))
                per_class[k] = (max(a, q), max(b, e))
    rep_r.done()
    rep_t.done()
    for k, (q, e) in sorted(per_class.items()):
        print(f"rbk_warp |r| = {rr.RBK_NORMS[k]:g}: worst error / bound = {q:.3f}, largest bound on a warped ray's element = {e:.3g}")


# ------------------------------------------------------------------------------------------------ positional encoding
def test_embed(L):
    rep = Report("embed")
    worst_u = 0.0
    for c in rr.cases_embed():
        n, dim = c["x"].shape
        x, out = T(c["x"]), Out(n, dim * (1 + 2 * c["L"]))
        ok(L, L.lib().evd_embed(L.ptr(x), n, dim, c["L"], out.ptr(), L.stream_ptr()), "evd_embed")
        got, fe = out.get(), rr.embed_arrays(LIFT, **c)
        assert same_bits(got[:, :dim], c["x"])
        worst_u = max(worst_u, float(np.abs(got - fe.value).max()) / fb.U)
        rep.inside(got, fe, rr.embed_arrays(F32, **c), (n, dim, c["L"]))
    print(f"embed: worst |sinf, cosf - float64| = {worst_u:.3f} u (K_TRIG = {fb.K_TRIG:g} u)")
    rep.done()


# ------------------------------------------------------------------------------------------------ backward of the ray packing
def test_ray_batch_bwd(L):
    rep = Report("ray_batch_bwd")
    for c in rr.cases_ray_batch_bwd():
        R = len(c["rays"])
        cfg = rcfg(L, c["H"], c["W"], c["focal"], c["ndc_on"], 1)
        g = c["g"].copy()
        g[:, 6:8] = np.nan                                        # the near / far columns carry no gradient: never read
        rays, gd, out = T(c["rays"]), T(g), Out(R, 3, 2)
        ok(L, L.lib().evd_ray_batch_bwd(C.byref(cfg), L.ptr(rays), L.ptr(gd), R, out.ptr(), L.stream_ptr()), "evd_ray_batch_bwd")
        rep.inside(out.get(), rr.ray_batch_bwd_arrays(LIFT, **c), rr.ray_batch_bwd_arrays(F32, **c), (R, c["ndc_on"]))
    rep.done()


# ------------------------------------------------------------------------------------------------ sample positions and their backward
def test_points_and_points_bwd(L):
    rep_f, rep_b, rep_a = Report("points"), Report("points_bwd overwrite"), Report("points_bwd accumulate")
    for c in rr.cases_points():
        R, S = c["z"].shape
        rb, z, g = T(c["rb"]), T(c["z"]), T(c["g"])
        pts = Out(R, S, 3)
        ok(L, L.lib().evd_points(L.ptr(rb), 11, L.ptr(z), R, S, pts.ptr(), L.stream_ptr()), "evd_points")
        rep_f.inside(pts.get(), rr.points_arrays(LIFT, c["rb"], c["z"]), rr.points_arrays(F32, c["rb"], c["z"]), (R, S))
        d = Out(R, 11)                                            # overwrite into NaN: the whole row is written
        ok(L, L.lib().evd_points_bwd(L.ptr(z), L.ptr(g), R, S, 0, d.ptr(), L.stream_ptr()), "evd_points_bwd")
        got = d.get()
        assert same_bits(got[:, 6:], np.zeros((R, 5), np.float32))
        rep_b.inside(got[:, :6], Fe(*rr.points_bwd_ref(c["z"], c["g"])), rr.points_bwd_f32(c["z"], c["g"]), (R, S))
        d = Out(R, 11, fill=c["prev"])                            # accumulate, twice: the other columns keep their bits
        prev = c["prev"][:, :6]
        for _ in range(2):
            ok(L, L.lib().evd_points_bwd(L.ptr(z), L.ptr(g), R, S, 1, d.ptr(), L.stream_ptr()), "evd_points_bwd")
            got = d.get()
            assert same_bits(got[:, 6:], c["prev"][:, 6:])
            rep_a.inside(got[:, :6], Fe(*rr.points_bwd_ref(c["z"], c["g"], prev)), rr.points_bwd_f32(c["z"], c["g"], prev), (R, S))
            prev = got[:, :6].copy()
    rep_f.done()
    rep_b.done()
    rep_a.done()


# ------------------------------------------------------------------------------------------------ the autograd nodes run these entries
@pytest.mark.parametrize("ndc_on", [True, False])
def test_ray_batch_train_backward_is_the_direct_call(L, ndc_on):
    from evdeblurnerf_amd.renderer import NeRFAll
    H, W, focal = rr.NDC_HWF
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]], np.float32)
    R = 257
    rs = np.random.RandomState(11)
    rays_h, g_h = rr.make_rays(rs, R), rs.standard_normal((R, 11)).astype(np.float32)
    cfg = rcfg(L, H, W, focal, ndc_on, 1)
    direct_rb, rays = Out(R, 11), T(rays_h)
    ok(L, L.lib().evd_ray_batch(C.byref(cfg), L.ptr(rays), R, direct_rb.ptr(), L.stream_ptr()), "evd_ray_batch")
    for g in (g_h, None):                                         # None: rb.sum().backward(), an expanded (non-contiguous) gradient
        leaf = T(rays_h).requires_grad_(True)
        rb = NeRFAll.ray_batch_train(H, W, K, leaf, ndc=ndc_on)
        assert same_bits(rb.detach().cpu().numpy(), direct_rb.get())
        if g is None:
            rb.sum().backward()
        else:
            rb.backward(T(g))
        direct = Out(R, 3, 2)
        gd = T(g_h if g is not None else np.ones((R, 11), np.float32))
        ok(L, L.lib().evd_ray_batch_bwd(C.byref(cfg), L.ptr(rays), L.ptr(gd), R, direct.ptr(), L.stream_ptr()), "evd_ray_batch_bwd")
        assert same_bits(leaf.grad.cpu().numpy(), direct.get())


def test_points_backward_is_the_direct_call(L):
    from evdeblurnerf_amd.renderer import points
    c = next(k for k in rr.cases_points() if k["z"].shape == (257, 65))
    R, S = c["z"].shape
    z = T(c["z"])
    for g in (c["g"], None):
        leaf = T(c["rb"]).requires_grad_(True)
        pts = points(leaf, z)
        direct_pts = Out(R, S, 3)
        ok(L, L.lib().evd_points(L.ptr(leaf.detach()), 11, L.ptr(z), R, S, direct_pts.ptr(), L.stream_ptr()), "evd_points")
        assert same_bits(pts.detach().cpu().numpy(), direct_pts.get())
        if g is None:
            pts.sum().backward()
        else:
            pts.backward(T(g))
        gd, direct = T(c["g"] if g is not None else np.ones((R, S, 3), np.float32)), Out(R, 11)
        ok(L, L.lib().evd_points_bwd(L.ptr(z), L.ptr(gd), R, S, 0, direct.ptr(), L.stream_ptr()), "evd_points_bwd")
        assert same_bits(leaf.grad.cpu().numpy(), direct.get())
