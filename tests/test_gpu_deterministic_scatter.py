"""The deterministic tri-plane scatter (evd_voxel_sample_bwd_det, csrc/kernel_voxel_scatter_det.hip) against the float64 reference of
tests/triplane_ref.py, and the properties it exists for: the same bits from run to run, under a permutation of the samples, across
accumulating calls and from a dirty workspace.

Error model: the one at the top of tests/test_gpu_triplane.py with kd = 12 + SPLIT / U + 2 F for d coef (here a float32 fmaf chain over F).
The float-atomic forms pay one float32 rounding per addition into a cell (cnt u M); this form adds in 64-bit fixed point, so a cell pays
  |got - ref| <= (kd + 4) u M + cnt unit
with at most half a unit of rounding per converted contribution, one float32 rounding of the converted sum and one of the addition into
the gradient.  unit = 2^(E_ref + 1 - (62 - ceil(log2(4 n)))): E_ref is the binary exponent (frexp) of the reference's largest magnitude
|d coef| x |other| over the batch -- line_row_max for the lines and the same maximum of dcom x lm for the planes; the entry takes ONE unit
per call from the float32 maximum of its own contributions, which is below that magnitude up to float32 rounding: one binade of slack.
d basis (12 + n / 16 + 64) and d pts (kd + 3 ct + 16) as the other forms."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import test_gpu_triplane as T
from evdeblurnerf_amd import _lib as L
from triplane_ref import MAT, VEC, _comp, src_indices, triplane

pytestmark = pytest.mark.gpu

F, U, AABB = T.F, T.U, T.AABB
SHAPES = ("shipped", "c12", "ct128")            # (64,16,16) hybrid-capable, (48,12,12) generic, (64,32,32) ct > 96
MODES = ("f32", "f16")                          # float32 grids / the float16 grid copies
KD = 12 + T.SPLIT / U + 2 * F


def run_det(lvl, mode, pts, d_out, planes, lines, basis, d_stride=F, d_col=0, dpts=True, basis_grad=True, into=None, dirty=False):
    """one call of the entry; into = (gp, gl, gb): accumulate into these tensors instead of fresh zeros"""
    n = pts.shape[0]
    p = torch.tensor(pts if n else np.zeros((1, 3), np.float32), device="cuda")
    g = torch.full((max(n, 1), d_stride), 7.0, dtype=torch.float32, device="cuda")
    g[:n, d_col:d_col + F] = torch.tensor(d_out, dtype=torch.float32)
    if into is None:
        gp = [torch.zeros(pl.shape, dtype=torch.float32, device="cuda") for pl in planes]
        gl = [torch.zeros(li.shape, dtype=torch.float32, device="cuda") for li in lines]
        gb = torch.zeros(basis.shape, dtype=torch.float32, device="cuda") if basis_grad else None
    else:
        gp, gl, gb = into
    gs = L.VoxelGridGrads()
    for i in range(3):
        gs.plane[i], gs.line[i] = gp[i].data_ptr(), gl[i].data_ptr()
    gs.basis = gb.data_ptr() if gb is not None else None
    dp = torch.full((max(n, 1), 3), np.nan, dtype=torch.float32, device="cuda") if dpts else None
    lib = L.lib()
    nb = int(lib.evd_voxel_sample_bwd_det_workspace_bytes(lvl.handle, n))
    assert nb > 0 or n == 0
    ws = torch.full((max(nb, 1),), 0xA5 if dirty else 0, dtype=torch.uint8, device="cuda")
    rc = lib.evd_voxel_sample_bwd_det(lvl.handle, L.PREC[mode], L.ptr(p), n, C.c_void_p(g.data_ptr()), d_stride, d_col, C.byref(gs), L.ptr(dp),
                                      L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, "evd_voxel_sample_bwd_det")
    torch.cuda.synchronize()
    return gp, gl, gb, dp


def unit_of(rp, rl, rb, src, d_out, r, n):
    """the test's unit (module docstring) from the reference's largest |d coef| x |other|"""
    f64 = lambda t: torch.as_tensor(t).to(device=rp[0].device, dtype=torch.float64)
    s = f64(src)
    dcom = f64(d_out).abs() @ rb.abs()
    m, off = float(r["line_row_max"]), 0
    for i in range(3):
        c = _comp(rp[i], rl[i], s[:, MAT[i][0]], s[:, MAT[i][1]], s[:, VEC[i]])
        Cn = rp[i].shape[2]
        m = max(m, float((dcom[:, off:off + Cn] * c["lm"]).max()))
        off += Cn
    if not m > 0:
        return 0.0
    e_ref = math.frexp(m)[1]
    k = 62 - math.ceil(math.log2(4 * n)) - (e_ref + 1)
    return 2.0 ** -min(k, 126)          # (the entry's clamp: evd_scatter_det_unit_exp)


def check_det(tag, r, unit, gp, gl, gb, dp, n, ct, src=None):
    w = {}
    for i in range(3):
        w[f"plane{i}"] = T.check(f"{tag} d plane {i}", gp[i], r["d_plane"][i], r["d_plane_m"][i], KD + 4,
                                 r["d_plane_cnt"][i].cpu() * unit * torch.ones_like(r["d_plane"][i].cpu()))
        w[f"line{i}"] = T.check(f"{tag} d line {i}", gl[i], r["d_line"][i], r["d_line_m"][i], KD + 4,
                                r["d_line_cnt"][i].cpu() * unit * torch.ones_like(r["d_line"][i].cpu()))
    if gb is not None:
        w["basis"] = T.check(f"{tag} d basis", gb, r["d_basis"], r["d_basis_m"], 12 + n / 16 + 64)
    if dp is not None:
        w["pts"] = T.check(f"{tag} d pts", dp[:n], r["d_pts"], r["d_pts_m"], KD + 3 * ct + 16, rows=None if src is None else [s.tolist() for s in src])
    return w


@functools.lru_cache(maxsize=None)
def case(shape, mode, si):
    """the level, inputs and float64 reference of (shape, mode, grid scale si): built once, shared by the tests, never modified"""
    scale = T.SCALES[si]
    lvl, gsz, planes, lines, basis = T.make_level(shape, "fine", scale, seed=7 + si)
    pts = T.points(gsz, 21 + si, n_rand=320)
    n = pts.shape[0]
    d_out = T.d_out_rows(np.random.RandomState(31 + si), n).astype(np.float32)
    src, kp = src_indices(pts, AABB, gsz)
    rp, rl, rb = T.ref_grids(planes, lines, basis, mode == "f16")
    r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
    unit = unit_of(rp, rl, rb, src, d_out, r, n)
    return dict(lvl=lvl, gsz=gsz, planes=planes, lines=lines, basis=basis, pts=pts, d_out=d_out, src=src, kp=kp, ref=r, unit=unit, refg=(rp, rl, rb))


def hot_cell(shape, mode, n=4096):
    """n points drawn uniformly inside ONE voxel: each of its tap cells receives thousands of contributions"""
    c = case(shape, mode, 1)
    rs = np.random.RandomState(77)
    gsz = c["gsz"]
    lo, hi = np.asarray(AABB[0]), np.asarray(AABB[1])
    cell = np.array([gsz[0] // 2, gsz[1] // 3, gsz[2] // 2])
    idx = cell + rs.uniform(0.05, 0.95, (n, 3))
    pts = (lo + idx / (np.array(gsz) - 1) * (hi - lo)).astype(np.float32)
    d_out = T.d_out_rows(rs, n).astype(np.float32)
    return c, pts, d_out


def bits_equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, (list, tuple)):
            if not bits_equal(x, y):
                return False
        elif x is None or y is None:
            if x is not y:
                return False
        elif not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            return False
    return True


# ---- 1. accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_det_scatter_matches_float64_reference(shape, mode):
    ct = sum(T.SHAPES[shape])
    worst = {}
    for si in range(len(T.SCALES)):
        c = case(shape, mode, si)
        n = c["pts"].shape[0]
        ds, dc = (40, 5) if si == 1 else (F, 0)             # strided d out rows on one scale
        gp, gl, gb, dp = run_det(c["lvl"], mode, c["pts"], c["d_out"], c["planes"], c["lines"], c["basis"], ds, dc, dpts=si != 3, basis_grad=si != 2)
        for key, v in check_det(f"{shape} {mode} scale {T.SCALES[si]:g}", c["ref"], c["unit"], gp, gl, gb, dp, n, ct, c["src"]).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"det {shape} {mode}: worst err / (u M):", " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 129])
@pytest.mark.parametrize("shape,mode", [("shipped", "f32"), ("c12", "f16")])
def test_det_scatter_ragged_n(shape, mode, n):
    c = case(shape, mode, 1)
    pts, d_out = c["pts"][-n:], c["d_out"][-n:]              # the tail: the random in-box points (the head is the edge cases)
    src, kp = src_indices(pts, AABB, c["gsz"])
    rp, rl, rb = c["refg"]
    r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
    gp, gl, gb, dp = run_det(c["lvl"], mode, pts, d_out, c["planes"], c["lines"], c["basis"], 40, 5)
    check_det(f"{shape} {mode} n {n}", r, unit_of(rp, rl, rb, src, d_out, r, n), gp, gl, gb, dp, n, sum(T.SHAPES[shape]), src)


def test_det_scatter_n_zero_is_a_no_op():
    c = case("shipped", "f32", 1)
    gp, gl, gb, dp = run_det(c["lvl"], "f32", np.zeros((0, 3), np.float32), np.zeros((0, F), np.float32), c["planes"], c["lines"], c["basis"])
    assert all(float(t.abs().sum()) == 0 for t in gp + gl + [gb])
    assert torch.isnan(dp).all()          # the (1, 3) stand-in buffer: not written


# ---- 2. run to run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which", ["hot_cell", "edge_case"])
def test_det_scatter_same_bits_from_run_to_run(which, shape, mode):
    if which == "hot_cell":
        c, pts, d_out = hot_cell(shape, mode)
    else:
        c = case(shape, mode, 1)
        pts, d_out = c["pts"], c["d_out"]
    runs = [run_det(c["lvl"], mode, pts, d_out, c["planes"], c["lines"], c["basis"]) for _ in range(3)]
    assert float(runs[0][0][0].abs().max()) > 0 and torch.isfinite(runs[0][3]).all()
    assert bits_equal(runs[0], runs[1]) and bits_equal(runs[0], runs[2])
    if which == "hot_cell":                 # ... and they are the right sums: thousands of contributions per cell
        n = pts.shape[0]
        src, kp = src_indices(pts, AABB, c["gsz"])
        rp, rl, rb = c["refg"]
        r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
        assert float(r["d_plane_cnt"][0].max()) > 1000
        check_det(f"hot cell {shape} {mode}", r, unit_of(rp, rl, rb, src, d_out, r, n), *runs[0], n, sum(T.SHAPES[shape]), src)


# ---- 3. permutation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_det_scatter_is_invariant_under_a_permutation_of_the_samples(shape, mode):
    c = case(shape, mode, 1)
    n = c["pts"].shape[0]
    perm = np.random.RandomState(5).permutation(n)
    gp, gl, gb, dp = run_det(c["lvl"], mode, c["pts"], c["d_out"], c["planes"], c["lines"], c["basis"])
    qp, ql, qb, dq = run_det(c["lvl"], mode, c["pts"][perm], c["d_out"][perm], c["planes"], c["lines"], c["basis"])
    assert bits_equal([gp, gl], [qp, ql])
    assert bits_equal([dp[torch.tensor(perm, device="cuda")]], [dq])
    T.check(f"{shape} {mode} permuted d basis", qb, c["ref"]["d_basis"], c["ref"]["d_basis_m"], 12 + n / 16 + 64)      # reproducible for a given order only


# ---- 4. accumulation, dirty workspace ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", [("shipped", "f16"), ("c12", "f32"), ("ct128", "f32")])
def test_det_scatter_accumulates_and_ignores_the_workspace_contents(shape, mode):
    c = case(shape, mode, 1)
    d2 = T.d_out_rows(np.random.RandomState(99), c["pts"].shape[0]).astype(np.float32)
    a = run_det(c["lvl"], mode, c["pts"], c["d_out"], c["planes"], c["lines"], c["basis"])
    b = run_det(c["lvl"], mode, c["pts"], d2, c["planes"], c["lines"], c["basis"])
    both = run_det(c["lvl"], mode, c["pts"], c["d_out"], c["planes"], c["lines"], c["basis"])
    both = run_det(c["lvl"], mode, c["pts"], d2, c["planes"], c["lines"], c["basis"], into=both[:3])
    want = ([x + y for x, y in zip(a[0], b[0])], [x + y for x, y in zip(a[1], b[1])], a[2] + b[2], b[3])
    assert bits_equal(want, both)
    dirty = run_det(c["lvl"], mode, c["pts"], c["d_out"], c["planes"], c["lines"], c["basis"], dirty=True)
    assert bits_equal(a, dirty)


# ---- 5. non-finite d out -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", [("shipped", "f32"), ("shipped", "f16"), ("ct128", "f32"), ("c12", "f32")])
def test_det_scatter_non_finite_d_out_takes_the_default_path(shape, mode):
    """one NaN row and one Inf row: no fixed-point scale exists; every gradient is finite exactly where evd_voxel_sample_bwd_prec's is, and
    the finite elements are within the bounds tests/test_gpu_triplane.py holds that entry to"""
    lvl, gsz, planes, lines, basis = T.make_level(shape, "fine", 0.1)
    rs = np.random.RandomState(4)
    n = 200
    pts = rs.uniform(np.array(AABB[0]) * 0.9, np.array(AABB[1]) * 0.9, (n, 3)).astype(np.float32)
    d_out = rs.normal(size=(n, F)).astype(np.float32)
    d_out[5, 9] = np.nan
    d_out[17, 3] = np.inf
    got = run_det(lvl, mode, pts, d_out, planes, lines, basis)
    dflt = T.run_bwd(lvl, "bwd_prec", mode, pts, d_out, planes=planes, lines=lines, basis=basis)
    for x, y in zip(got[0] + got[1] + [got[2], got[3]], dflt[0] + dflt[1] + [dflt[2], dflt[3]]):
        assert torch.equal(torch.isfinite(x), torch.isfinite(y))
    kernel = T.bwd_kernel(shape, "bwd_prec", T.MODES[mode][1], True)
    rp, rl, rb = T.ref_grids(planes, lines, basis, T.bwd_half(kernel, "bwd_prec", mode))
    src, kp = src_indices(pts, AABB, gsz)
    r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
    assert not torch.isfinite(r["d_basis"]).all() and not torch.isfinite(r["d_line"][0]).all()
    T.check_bwd(kernel, kernel, r, *got, n, sum(T.SHAPES[shape]))
