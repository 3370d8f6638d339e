"""The ray front end restated once, generic in the number type.  Test infrastructure only.

Every function below is plain arithmetic on "numbers" that may be
  * fe_bound.Fe                         -> the exact value and a bound on a float32 evaluation's distance from it,
  * float32 numpy arrays (>= 1-d)       -> the stand-in for a correct kernel (one IEEE rounding per operation),
  * float64 torch tensors               -> autograd.
The formulas are those of the reference (utils/rays.py:8-36 camera model, :104-145 NDC warp; networks/renderer.py:423-446 ray packing;
networks/embedding.py:88-98 positional encoding; networks/dpnerf/blurmodel.py:51-82 with utils/rigid_warping.py:18-49,72-132 the SE(3)
exponential of the sub-exposure poses), in the operation order that the comments of csrc/kernels_rays.hip and csrc/ray_math.h state.  Vectors are lists of
components, so that nothing here depends on an array library's stacking; `cols` / fe_bound.stack go between the two forms.  Scalars that
the reference holds as Python doubles and rounds to float32 when they meet a tensor (cw, ch, 2 near, 1e-10) are Python floats that are
float32 numbers.

points_bwd_* are not generic: the kernel's summation shape gives its bound in closed form."""
import math

import numpy as np

from fe_bound import Fe, U, concat, stack

F32 = np.float32
EPS_THETA = float(F32(1.0e-10))


def f32(a):
    """float32 array of at least one dimension (numpy's scalars promote differently from arrays)"""
    return np.atleast_1d(np.asarray(a, dtype=F32))


def cols(a, n=None):
    """[..., n] -> list of n components"""
    return [a[..., c] for c in range(a.shape[-1] if n is None else n)]


def _sqrt(x):
    return x.sqrt() if hasattr(x, "sqrt") else np.sqrt(x)


def _sin(x):
    # (the float32 stand-in rounds the float64 function: a correctly rounded sinf, the same on every CPU)
    return x.sin() if hasattr(x, "sin") else np.sin(x.astype(np.float64)).astype(F32)


def _cos(x):
    return x.cos() if hasattr(x, "cos") else np.cos(x.astype(np.float64)).astype(F32)


def ndc_coeffs(H, W, focal):
    """utils/rays.py:135-140: Python doubles, rounded to float32 where they meet the tensor"""
    return float(F32(-1.0 / (W / (2.0 * float(focal))))), float(F32(-1.0 / (H / (2.0 * float(focal)))))


# ---------------------------------------------------------------------------------------------- camera model, utils/rays.py:8-36
def camera_rays(x, y, K, c, add_halfpix=True):
    """pixel positions x (column), y (row); K = (k00, k02, k11, k12); c = the 12 entries of the pose [3,4], each a number that broadcasts
    against x -> (o, d).  d = c2w[:3,:3] . ((x + (h - k02)) / k00, -(y + (h - k12)) / k11, -1), summed left to right."""
    k00, k02, k11, k12 = K
    h = 0.5 if add_halfpix else 0.0
    d0 = (x + (h - k02)) / k00
    d1 = -((y + (h - k12)) / k11)
    d = [(d0 * c[r * 4] + d1 * c[r * 4 + 1]) + (-c[r * 4 + 2]) for r in range(3)]
    o = [c[r * 4 + 3] for r in range(3)]
    return o, d


def pixel_grid(H, W):
    """(column, row) of the H W pixels in row-major order, float32"""
    idx = np.arange(H * W)
    return f32(idx % W), f32(idx // W)


def get_rays(num, H, W, K, c2w, add_halfpix=True):
    """utils/rays.py:8-22.  num: float32 array -> number.  K [3,3], c2w [3,4] float32 -> (o, d), lists of [H W] components"""
    x, y = pixel_grid(H, W)
    K, c2w = f32(K), f32(c2w).reshape(-1)
    Kn = [num(f32(K[0, 0])), num(f32(K[0, 2])), num(f32(K[1, 1])), num(f32(K[1, 2]))]
    return camera_rays(num(x), num(y), Kn, [num(f32(v)) for v in c2w[:12]], add_halfpix)


def get_rays_pix(num, coords, K, c2ws, add_halfpix=True):
    """utils/rays.py:25-36.  coords [n,2], c2ws [n,3,4]: a pose per ray"""
    K, c2ws, coords = f32(K), f32(c2ws).reshape(len(coords), -1), f32(coords)
    Kn = [num(f32(K[0, 0])), num(f32(K[0, 2])), num(f32(K[1, 1])), num(f32(K[1, 2]))]
    return camera_rays(num(coords[:, 0]), num(coords[:, 1]), Kn, [num(c2ws[:, k]) for k in range(12)], add_halfpix)


# ---------------------------------------------------------------------------------------------- NDC warp, utils/rays.py:104-145
def ndc(cw, ch, near, o, d):
    two_near = float(F32(2.0 * float(near)))
    near = float(F32(near))
    t = -(near + o[2]) / d[2]
    ox, oy, oz = o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]
    ox_oz, oy_oz = ox / oz, oy / oz
    o2 = 1.0 + two_near / oz
    return [cw * ox_oz, ch * oy_oz, o2], [cw * (d[0] / d[2] - ox_oz), ch * (d[1] / d[2] - oy_oz), 1.0 - o2]


# ---------------------------------------------------------------------------------------------- ray packing, networks/renderer.py:423-446
def ray_batch(o, d, cw, ch, ndc_on=True, use_viewdirs=True, ndc_near=1.0):
    """-> (o', d', viewdirs or None): columns 0..2, 3..5 and 8..10 of the packed row (6, 7 are near / far, copied).  viewdirs = d / |d|
    BEFORE the warp (:431); the warp's near plane is 1 (:437)."""
    vd = None
    if use_viewdirs:
        nrm = _sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        vd = [d[c] / nrm for c in range(3)]
    if ndc_on:
        o, d = ndc(cw, ch, ndc_near, o, d)
    return list(o), list(d), vd


def pack(o, d, near, far, vd):
    """the [R, 8 or 11] row from ray_batch's parts, Fe or float32 (near / far are float32 numbers, copied)"""
    shape = o[0].shape
    const = (lambda c: Fe(np.full(shape, float(F32(c))))) if isinstance(o[0], Fe) else (lambda c: np.full(shape, c, F32))
    return stack(list(o) + list(d) + [const(near), const(far)] + (list(vd) if vd is not None else []), -1)


def ray_batch_bwd(o, d, g, cw, ch, ndc_on=True, drop=()):
    """Closed form of the packing's backward as k_ray_batch_bwd evaluates it: g = the 11 columns of the upstream gradient (6, 7 unused)
    -> (d loss / d o, d loss / d d).  With o' = o + t d, t = -(1 + o_z) / d_z, a = o'_z:  o_out = (cw o'_x / a, ch o'_y / a, 1 + 2 / a),
    d_out = (cw (d_x / d_z - o'_x / a), ch (d_y / d_z - o'_y / a), -2 / a), viewdirs = d / |d|.
    `drop` names terms to leave out, for the planted-fault tests only: "gt_dz2" (the g_t (1 + o_z) / d_z^2 term of gd[2]), "proj" (the
    view directions' projection d (g . d) / |d|^2)."""
    goo, gdo, gv = g[0:3], g[3:6], g[8:11]
    if ndc_on:
        t = -(1.0 + o[2]) / d[2]
        px, py, a = o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]
        ia, idz = 1.0 / a, 1.0 / d[2]
        g_ox, g_oy = cw * (goo[0] - gdo[0]), ch * (goo[1] - gdo[1])
        gp = [g_ox * ia, g_oy * ia, ((2.0 * (gdo[2] - goo[2]) - g_ox * px) - g_oy * py) * ia * ia]
        g_t = (gp[0] * d[0] + gp[1] * d[1]) + gp[2] * d[2]
        go = [gp[0], gp[1], gp[2] - g_t * idz]
        gd = [t * gp[0] + cw * gdo[0] * idz, t * gp[1] + ch * gdo[1] * idz,
              t * gp[2] - (cw * gdo[0] * d[0] + ch * gdo[1] * d[1]) * idz * idz]
        if "gt_dz2" not in drop:
            gd[2] = gd[2] + g_t * (1.0 + o[2]) * idz * idz
    else:
        go, gd = list(goo), list(gdo)
    n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    inr = 1.0 / _sqrt(n2)
    dot = ((gv[0] * d[0] + gv[1] * d[1]) + gv[2] * d[2]) / n2
    for c in range(3):
        gd[c] = gd[c] + ((gv[c] - d[c] * dot) if "proj" not in drop else gv[c]) * inr
    return go, gd


# ---------------------------------------------------------------------------------------------- rbk_warp, blurmodel.py:51-82
def split_motion(r, M):
    """r [R, 3 M] as the reference views it, [R, 3, M] (blurmodel.py:52-53) -> 3 components of [R, M]"""
    r3 = r.reshape(r.shape[0], 3, M)
    return [r3[:, c, :] for c in range(3)]


def se3_exp(rot, tr):
    """SE3Field.get_transform (rigid_warping.py:18-30) over RigidBody.exp_se3 / exp_so3 (:72-110): rot, tr = 3 components each ->
    T, 3 rows of 4 numbers.  theta = |rot| + 1e-10; w = rot / theta, v = tr / theta; W = skew(w);
    R = I + sin(theta) W + (1 - cos(theta)) W W;  p = (theta I + (1 - cos(theta)) W + (theta - sin(theta)) W W) v"""
    theta = _sqrt((rot[0] * rot[0] + rot[1] * rot[1]) + rot[2] * rot[2]) + EPS_THETA
    w = [rot[c] / theta for c in range(3)]
    v = [tr[c] / theta for c in range(3)]
    Wm = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    W2 = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + Wm[a][k] * Wm[k][b]
            W2[a][b] = acc
    st, omc = _sin(theta), 1.0 - _cos(theta)
    tms = theta - st
    T = [[None] * 4 for _ in range(3)]
    for a in range(3):
        p = 0.0
        for b in range(3):
            eye = 1.0 if a == b else 0.0
            T[a][b] = (eye + st * Wm[a][b]) + omc * W2[a][b]
            g = (theta * eye + omc * Wm[a][b]) + tms * W2[a][b]
            p = p + g * v[b]
        T[a][3] = p
    return T


def rbk_warp(o, d, rot, tr):
    """one sub-exposure slot per element: o, d, rot, tr = 3 components each, broadcasting against each other -> (o', d', T).
    o' = T o, d' = T (o + d) - T o (blurmodel.py:56,70-72)"""
    T = se3_exp(rot, tr)
    e = [o[c] + d[c] for c in range(3)]
    wo = [((T[a][0] * o[0] + T[a][1] * o[1]) + T[a][2] * o[2]) + T[a][3] for a in range(3)]
    we = [((T[a][0] * e[0] + T[a][1] * e[1]) + T[a][2] * e[2]) + T[a][3] for a in range(3)]
    return wo, [we[a] - wo[a] for a in range(3)], T


def rbk_warp_arrays(num, rays, r, v, M, use_origin, split=split_motion):
    """rays [R,3,2], r, v [R,3 M] float32 -> (new_rays [R,P,3,2], transforms [R,P,4,4]) in the number type of `num` (Fe or float32),
    the origin slot and the transforms' last row being exact copies / constants"""
    rays, r, v = f32(rays), f32(r), f32(v)
    R = rays.shape[0]
    o = [num(rays[:, c, 0][:, None]) for c in range(3)]
    d = [num(rays[:, c, 1][:, None]) for c in range(3)]
    wo, wd, T = rbk_warp(o, d, [num(x) for x in split(r, M)], [num(x) for x in split(v, M)])
    const = lambda c: num(np.full((R, M), c, F32))
    nr = stack([stack([wo[c], wd[c]], -1) for c in range(3)], -2)                                  # [R,M,3,2]
    tf = stack([stack(T[a], -1) for a in range(3)] + [stack([const(0.0)] * 3 + [const(1.0)], -1)], -2)   # [R,M,4,4]
    if use_origin:
        nr = concat([num(rays[:, None]), nr], 1)
        tf = concat([num(np.broadcast_to(np.eye(4, dtype=F32), (R, 1, 4, 4)).copy()), tf], 1)
    return nr, tf


# ---------------------------------------------------------------------------------------------- positional encoding, embedding.py:88-98
def embed(x, L, swap=False):
    """x [n, dim] -> the 1 + 2 L blocks [x, sin x, cos x, sin 2x, cos 2x, ...]; x 2^k is exact in float32, so the Fe value is sin / cos of the
    float64 product.  swap: cos before sin (planted-fault tests only)."""
    out = [x]
    for k in range(L):
        a = x * float(2 ** k)
        out += [_cos(a), _sin(a)] if swap else [_sin(a), _cos(a)]
    return out


# ---------------------------------------------------------------------------------------------- sample positions, renderer.py:180
def points(o, d, z):
    """pts = o + d z: o, d = 3 components of [R,1], z [R,S] -> 3 components of [R,S]"""
    return [o[c] + d[c] * z for c in range(3)]


def points_bwd_ref(z, g, prev=None):
    """float64 value and bound of k_points_bwd's six sums.  z [R,S], g [R,S,3] float32; prev [R,6] float32 = what the buffer held, when
    accumulating -> (value [R,6], bound [R,6]); columns 0..2 = sum_s g, 3..5 = sum_s z g.
    The kernel: per lane a serial sum over ceil(S/64) samples, six butterfly steps over the wavefront, one product in the z columns:
    at most ceil(S/64) + 6 roundings on any term, + 1 for the addition into the buffer."""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    S = z.shape[1]
    terms = np.concatenate([g, z[..., None] * g], -1)                   # [R,S,6]
    val, mag = terms.sum(1), np.abs(terms).sum(1)
    n = math.ceil(S / 64) + 6
    if prev is None:
        return val, n * U * mag
    prev = np.asarray(prev, np.float64)
    return val + prev, (n + 1) * U * (mag + np.abs(prev))


def points_bwd_f32(z, g, prev=None, steps=(32, 16, 8, 4, 2, 1), assign=False):
    """float32 restatement of k_points_bwd's summation (lane l sums samples l, l + 64, ...; butterfly; lane q holds column q).  `steps`
    short of six, or `assign` (= for += when accumulating), are the planted faults."""
    z, g = f32(z), f32(g)
    R, S = z.shape
    terms = np.concatenate([g, z[..., None] * g], -1)                   # float32 products
    a = np.zeros((R, 64, 6), F32)
    for s0 in range(0, S, 64):
        blk = terms[:, s0:s0 + 64]
        a[:, :blk.shape[1]] = a[:, :blk.shape[1]] + blk
    lane = np.arange(64)
    for off in steps:
        a = a + a[:, lane ^ off]
    out = np.stack([a[:, q, q] for q in range(6)], -1)
    if prev is None or assign:
        return out
    return f32(prev) + out


# ---------------------------------------------------------------------------------------------- array forms (Fe or float32, by `num`)
def get_rays_arrays(num, H, W, K, c2w, add_halfpix=True):
    o, d = get_rays(num, H, W, K, c2w, add_halfpix)
    return stack([x if x.shape == (H * W,) else _spread(x, H * W) for x in o], -1), stack(d, -1)


def _spread(x, n):
    return Fe(np.broadcast_to(x.value, (n,)), np.broadcast_to(x.err, (n,))) if isinstance(x, Fe) else np.broadcast_to(x, (n,))


def get_rays_pix_arrays(num, coords, K, c2ws, add_halfpix=True):
    o, d = get_rays_pix(num, coords, K, c2ws, add_halfpix)
    return stack(o, -1), stack(d, -1)


def ndc_arrays(num, H, W, focal, near, o, d):
    cw, ch = ndc_coeffs(H, W, focal)
    oo, od = ndc(cw, ch, near, cols(num(f32(o))), cols(num(f32(d))))
    return stack(oo, -1), stack(od, -1)


def ray_batch_arrays(num, H, W, focal, rays, ndc_on, use_viewdirs, near, far, ndc_near=1.0):
    """rays [R,3,2] float32 -> [R, 8 or 11]"""
    cw, ch = ndc_coeffs(H, W, focal)
    rays = num(f32(rays))
    o, d, vd = ray_batch(cols(rays[..., 0]), cols(rays[..., 1]), cw, ch, ndc_on, use_viewdirs, ndc_near)
    return pack(o, d, near, far, vd)


def ray_batch_bwd_arrays(num, H, W, focal, rays, g, ndc_on, drop=()):
    """rays [R,3,2], g [R,11] float32 (columns 6, 7 are not read) -> d rays [R,3,2]"""
    cw, ch = ndc_coeffs(H, W, focal)
    rays, g = num(f32(rays)), f32(g).copy()
    g[:, 6:8] = 0
    go, gd = ray_batch_bwd(cols(rays[..., 0]), cols(rays[..., 1]), cols(num(g)), cw, ch, ndc_on, drop)
    return stack([stack([go[c], gd[c]], -1) for c in range(3)], -2)


def embed_arrays(num, x, L, swap=False):
    return concat(embed(num(f32(x)), L, swap), -1)


def points_arrays(num, rb, z):
    rb, z = f32(rb), f32(z)
    p = points([num(rb[:, c:c + 1]) for c in range(3)], [num(rb[:, 3 + c:4 + c]) for c in range(3)], num(z))
    return stack(p, -1)


# ---------------------------------------------------------------------------------------------- the inputs both test files use
K_TEST = np.array([[351.7, 0.0, 148.3], [0.0, 347.2, 201.9], [0.0, 0.0, 1.0]], F32)      # fx != fy, a fractional off-centre principal point
NDC_HWF = (300, 400, 350.0)
GET_RAYS_HW = ((1, 1), (7, 5), (17, 300), (60, 80))
COUNTS = (1, 255, 256, 257)
RBK_NORMS = (0.0, 1e-6, 1e-3, 1e-2, 0.3, 3.1, 6.5)


def make_pose(rs, n=None):
    """[3,4] (or [n,3,4]) float32: a random rotation (no zero entry) and a translation"""
    q, _ = np.linalg.qr(rs.standard_normal((n or 1, 3, 3)))
    p = np.concatenate([q, rs.standard_normal((n or 1, 3, 1)) * 2.0], -1).astype(F32)
    assert np.all(p != 0)
    return p if n else p[0]


def make_coords(rs, n):
    """fractional and negative pixel positions"""
    return rs.uniform(-30.0, 430.0, (n, 2)).astype(F32)


def make_rays(rs, R):
    """[R,3,2]: d_z of both signs with |d_z| >= 0.05 |d|, |d| in {1e-3, 1, 1e3} by ray (|d_z| >= 0.05 where |d| = 1), origins on both
    sides of the planes z = -1 and z = -0.5"""
    d = rs.standard_normal((R, 3))
    d[:, 2] = np.where(rs.uniform(size=R) < 0.5, -1.0, 1.0) * rs.uniform(0.06, 1.5, R) * np.linalg.norm(d[:, :2], axis=1).clip(0.2)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.array([1.0, 1e-3, 1e3])[np.arange(R) % 3][:, None]
    o = rs.standard_normal((R, 3))
    o[:, 2] = rs.uniform(-3.0, 1.5, R)
    rays = np.stack([o, d], -1).astype(F32)
    dz, dn = rays[:, 2, 1].astype(np.float64), np.linalg.norm(rays[:, :, 1].astype(np.float64), axis=1)
    assert np.all(np.abs(dz) >= 0.05 * dn)
    return rays


def make_rbk(rs, R, M, offset=0):
    """rays [R,3,2], r, v [R,3 M] (the [R,3,M] layout): |r| per ray from RBK_NORMS (0 exactly included), |v| in {1e-2, 1}, a direction of
    its own in every motion slot -> (rays, r, v, class index per ray)"""
    cls = (np.arange(R) + offset) % len(RBK_NORMS)
    vn = np.where((np.arange(R) // len(RBK_NORMS)) % 2 == 0, 1e-2, 1.0)
    def dirs():
        u = rs.standard_normal((R, 3, M))
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    r = (dirs() * np.asarray(RBK_NORMS)[cls][:, None, None]).astype(F32).reshape(R, 3 * M)
    v = (dirs() * vn[:, None, None]).astype(F32).reshape(R, 3 * M)
    rays = rs.standard_normal((R, 3, 2)).astype(F32)
    return rays, r, v, cls


def cases_get_rays():
    for k, (H, W) in enumerate(GET_RAYS_HW):
        for hp in (True, False):
            yield dict(H=H, W=W, K=K_TEST, c2w=make_pose(np.random.RandomState(100 + k)), add_halfpix=hp)


def cases_get_rays_pix():
    for n in COUNTS:
        rs = np.random.RandomState(200 + n)
        for hp in (True, False):
            yield dict(coords=make_coords(rs, n), K=K_TEST, c2ws=make_pose(rs, n), add_halfpix=hp)


def cases_ndc():
    H, W, focal = NDC_HWF
    for R in COUNTS:
        for near in (1.0, 0.5):
            rays = make_rays(np.random.RandomState(300 + R), R)
            yield dict(H=H, W=W, focal=focal, near=near, o=rays[..., 0].copy(), d=rays[..., 1].copy())


def cases_ray_batch():
    H, W, focal = NDC_HWF
    for R in COUNTS:
        for uv in (1, 0):
            for on in (1, 0):
                yield dict(H=H, W=W, focal=focal, rays=make_rays(np.random.RandomState(400 + R), R), ndc_on=on, use_viewdirs=uv, near=0.25, far=7.5)


def cases_rbk():
    for R in (1, 29, 257):
        for M in (1, 9):
            for uo in (1, 0):
                rays, r, v, cls = make_rbk(np.random.RandomState(500 + R + M), R, M, offset=3 if (R == 1 and M == 9) else 0)
                yield dict(rays=rays, r=r, v=v, M=M, use_origin=uo), cls


def cases_embed():
    for L in (0, 1, 4, 10):
        for dim in (1, 3, 4):
            for n in (1, 85, 86):
                for amp in (1.5, 40.0):
                    yield dict(x=np.random.RandomState(600 + n + dim).uniform(-amp, amp, (n, dim)).astype(F32), L=L)


def cases_ray_batch_bwd():
    """the upstream gradient: random normal, then the eleven one-hot columns"""
    H, W, focal = NDC_HWF
    for R in (1, 256, 257):
        rs = np.random.RandomState(700 + R)
        rays = make_rays(rs, R)
        gs = [rs.standard_normal((R, 11)).astype(F32)] + [np.eye(11, dtype=F32)[c][None].repeat(R, 0) for c in range(11)]
        for on in (1, 0):
            for g in gs:
                yield dict(H=H, W=W, focal=focal, rays=rays, g=g, ndc_on=on)


def cases_points():
    for S in (1, 63, 64, 65, 128, 200):
        for R in (1, 3, 4, 5, 257):
            rs = np.random.RandomState(800 + S + R)
            yield dict(rb=rs.standard_normal((R, 11)).astype(F32), z=np.sort(rs.uniform(0.0, 6.0, (R, S)), -1).astype(F32),
                       g=rs.standard_normal((R, S, 3)).astype(F32), prev=rs.standard_normal((R, 11)).astype(F32))
