"""Every form of the tri-plane gather (evd_voxel_sample / _prec) and scatter (evd_voxel_sample_bwd / _ws / _prec) against the float64
reference of tests/triplane_ref.py, element by element: |kernel - ref| <= k 2^-p M with M the same expression on absolute values, and
isfinite(kernel) == isfinite(ref).  The forms are reached by shape and mode only, as launch_voxel_sample, voxel_scatter_hybrid_ok,
voxel_sample_bwd_w_ok and launch_sample_bwd_block dispatch them; each case id names the kernel it expects.

Error model (u = 2^-24; ct = sum(n_comp), F = app_dim = 32; cnt = float additions into one gradient cell):
  interpolation + coefficient            pv, lv: <= 4 + 2 float32 steps, coef = pv lv: 1                      -> 12 u
  float32 basis GEMM (w / block forms)   an fmaf chain over ct                                                 -> ct u
  split-float16 product (m form, and     both operands power-of-two scaled into [2^13, 2^14), hi + lo; the
    every scatter's d coef)              dropped lo x lo and the two lo roundings: 3 x 2^-22 per product, one
                                         float32 rounding per MFMA into the accumulator                        -> 3 x 2^-22 + steps u
  plane / line / basis gradient          + one float32 rounding per addition into the cell (atomics, register
                                         sums): cnt u; line cells in fixed point: + cnt 2^-49 max |line row|
  d pts                                  + 3 ct float32 steps over the channels and components
"""
import ctypes as C

import numpy as np
import pytest
import torch

from evdeblurnerf_amd import _lib as L, weights as W
from evdeblurnerf_amd.voxnerf import VoxelNeRFBase
from triplane_ref import edge_points, f16_copy, index_points, src_indices, triplane

pytestmark = pytest.mark.gpu

AABB = ([-1.5, -1.5, -1.0], [1.5, 1.5, 1.0])
U = 2.0 ** -24
SPLIT = 3 * 2.0 ** -22
SCALES = (2.0 ** -10, 0.1, 1.0, 2.0 ** 10)
F = 32

# n_comp -> (is every component a multiple of 8, ct % 32 == 0 and ct <= 96, every component in {16, 32, 64})
SHAPES = {"shipped": (64, 16, 16), "ct80": (32, 16, 32), "c12": (48, 12, 12), "ct128": (64, 32, 32), "c16": (16, 16, 16)}
# a mode's level and whether its gather reads the float16 grid copies (voxel_net.h grids_half_for): f16c on the FINE level of a
# c2f pair (a level fed by the previous one: ft_dim 64 > app_dim) reads them, on the coarse level it does not
MODES = {"f32": ("fine", False), "f16x3": ("fine", False), "f16": ("fine", True), "bf16": ("fine", True), "f16c": ("fine", True),
         "f16c_coarse": ("coarse", False)}


def fwd_kernel(shape, half):
    nc = SHAPES[shape]
    ct = sum(nc)
    if all(c % 8 == 0 for c in nc):
        if half and ct % 32 == 0 and ct <= 96:
            return "k_voxel_sample_m"
        return "k_voxel_sample_w<true,4>" if half else "k_voxel_sample_w<false,3>"
    return f"k_voxel_sample<{'true' if half else 'false'},4>"


def bwd_kernel(shape, entry, half, dpts):
    nc = SHAPES[shape]
    ct = sum(nc)
    mm = ct % 32 == 0
    hybrid = entry != "bwd" and all(c in (16, 32, 64) for c in nc)
    if hybrid and ct % 32 == 0 and ct <= 96:
        return f"k_voxel_sample_bwd_w<{'true' if dpts else 'false'},{'true' if half else 'false'}>+k_scatter_lines"
    k = f"k_voxel_sample_bwd<{'true' if hybrid else 'false'},{'true' if mm else 'false'},{96 if mm and ct <= 96 else 128}>"
    return k + ("+k_scatter_lines" if hybrid else "")


def fwd_bound(kernel, ct):
    """k 2^-p of a forward form, as a multiple of u"""
    if kernel.startswith("k_voxel_sample_m"):
        return 12 + 3 * (ct // 32) * 3 + SPLIT / U
    return 12 + ct


def make_level(shape, kind, scale, seed=3, grids=None, nvox=20 ** 3):
    nc = SHAPES[shape] if isinstance(shape, str) else shape
    gsz = W.pdrf_grid_size(AABB[0], AABB[1], nvox)
    net = dict(input_ch=127, hidden_dim=256, geo_feat_dim=128) if kind == "fine" else dict(input_ch=95, hidden_dim=64, geo_feat_dim=15)
    sd = W.make_pdrf_state_dict(seed, gsz, app_n_comp=nc, grid_scale=scale, **net)
    if grids is not None:
        sd.update(grids(sd))
    lvl = VoxelNeRFBase(sd, "", AABB, app_n_comp=nc, n_voxels=nvox, rgb_activate="none" if kind == "fine" else "relu", **net)
    planes = [np.ascontiguousarray(np.asarray(sd[f"app_plane.{i}"], np.float32)[0].transpose(1, 2, 0)) for i in range(3)]
    lines = [np.ascontiguousarray(np.asarray(sd[f"app_line.{i}"], np.float32)[0, :, :, 0].T) for i in range(3)]
    basis = np.asarray(sd["basis_mat.weight"], np.float32)
    return lvl, gsz, planes, lines, basis


def run_fwd(lvl, mode, pts, out_stride=F, out_col=0, sentinel=None):
    n = pts.shape[0]
    p = torch.tensor(pts, device="cuda")
    out = torch.full((max(n, 1), out_stride), np.nan if sentinel is None else sentinel, dtype=torch.float32, device="cuda")
    if mode is None:
        rc = L.lib().evd_voxel_sample(lvl.handle, L.ptr(p), n, C.c_void_p(out.data_ptr()), out_stride, out_col, L.stream_ptr())
    else:
        prec = L.PREC["f16c" if mode.startswith("f16c") else mode]
        rc = L.lib().evd_voxel_sample_prec(lvl.handle, prec, L.ptr(p), n, C.c_void_p(out.data_ptr()), out_stride, out_col, L.stream_ptr())
    L.check(rc, "sample")
    torch.cuda.synchronize()
    return out


def run_bwd(lvl, entry, mode, pts, d_out, d_stride=F, d_col=0, dpts=True, basis_grad=True, planes=None, lines=None, basis=None):
    n = pts.shape[0]
    p = torch.tensor(pts if n else np.zeros((1, 3), np.float32), device="cuda")
    g = torch.full((max(n, 1), d_stride), 7.0, dtype=torch.float32, device="cuda")
    g[:n, d_col:d_col + F] = torch.tensor(d_out, dtype=torch.float32)
    gp = [torch.zeros(pl.shape, dtype=torch.float32, device="cuda") for pl in planes]
    gl = [torch.zeros(li.shape, dtype=torch.float32, device="cuda") for li in lines]
    gb = torch.zeros(basis.shape, dtype=torch.float32, device="cuda") if basis_grad else None
    gs = L.VoxelGridGrads()
    for i in range(3):
        gs.plane[i], gs.line[i] = gp[i].data_ptr(), gl[i].data_ptr()
    gs.basis = gb.data_ptr() if gb is not None else None
    dp = torch.full((max(n, 1), 3), np.nan, dtype=torch.float32, device="cuda") if dpts else None
    lib = L.lib()
    if entry == "bwd":
        rc = lib.evd_voxel_sample_bwd(lvl.handle, L.ptr(p), n, C.c_void_p(g.data_ptr()), d_stride, d_col, C.byref(gs), L.ptr(dp), L.stream_ptr())
    else:
        nb = int(lib.evd_voxel_sample_bwd_workspace_bytes(lvl.handle, n))
        ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device="cuda")
        if entry == "bwd_ws":
            rc = lib.evd_voxel_sample_bwd_ws(lvl.handle, L.ptr(p), n, C.c_void_p(g.data_ptr()), d_stride, d_col, C.byref(gs), L.ptr(dp), L.ptr(ws), nb,
                                             L.stream_ptr())
        else:
            prec = L.PREC["f16c" if mode.startswith("f16c") else mode]
            rc = lib.evd_voxel_sample_bwd_prec(lvl.handle, prec, L.ptr(p), n, C.c_void_p(g.data_ptr()), d_stride, d_col, C.byref(gs), L.ptr(dp),
                                               L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, entry)
    torch.cuda.synchronize()
    return gp, gl, gb, dp


def check(name, got, ref, mag, k, extra=None, rows=None):
    """element by element: finite where the reference is, and |got - ref| <= k u M (+ extra) there; returns the worst err / (u M).
    rows: per-row context (e.g. the source indices) shown for the worst elements of a failure"""
    got, ref, mag = got.detach().double().cpu(), ref.double().cpu(), mag.double().cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), f"{name}: finiteness differs at {int((torch.isfinite(got) != fin).sum())} elements"
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    bound = (k * U * mag + (extra if extra is not None else 0)).expand_as(mag)
    ratio = err / (U * mag + 1e-300)
    worst = float(ratio.max()) if err.numel() else 0.0
    bad = err > bound
    if bad.any():
        idx = torch.nonzero(bad)[:6]
        info = "; ".join(f"{tuple(i.tolist())}: got {float(got[tuple(i)]):.6g} ref {float(ref[tuple(i)]):.6g} M {float(mag[tuple(i)]):.3g}"
                         + (f" row {rows[int(i[0])]}" if rows is not None else "") for i in idx)
        raise AssertionError(f"{name}: {int(bad.sum())} elements over the bound, worst err / (u M) = {worst:.3g} (k = {float(torch.as_tensor(k).max()):.3g}): {info}")
    return worst


def points(gsz, seed, n_rand=160):
    rs = np.random.RandomState(seed)
    return edge_points(AABB, gsz, rs, n_rand=n_rand)


def ref_grids(planes, lines, basis, half):
    cv = (lambda a: f16_copy(torch.tensor(a))) if half else (lambda a: torch.tensor(a, dtype=torch.float64))
    return [cv(p) for p in planes], [cv(l) for l in lines], torch.tensor(basis, dtype=torch.float64)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
FWD_CASES = [(s, m, fwd_kernel(s, MODES[m][1])) for s in SHAPES for m in MODES] + [(s, "sample", fwd_kernel(s, False)) for s in SHAPES]


@pytest.mark.parametrize("shape,mode,kernel", FWD_CASES, ids=[f"{s}-{m}-{k}" for s, m, k in FWD_CASES])
def test_gather_matches_float64_reference(shape, mode, kernel):
    kind, half = MODES.get(mode, ("fine", False))
    ct = sum(SHAPES[shape])
    k = fwd_bound(kernel, ct)
    worst = []
    for si, scale in enumerate(SCALES):
        lvl, gsz, planes, lines, basis = make_level(shape, kind, scale, seed=5 + si)
        pts = points(gsz, 11 + si)
        src, _ = src_indices(pts, AABB, gsz)
        out = run_fwd(lvl, None if mode == "sample" else mode, pts)
        rp, rl, rb = ref_grids(planes, lines, basis, half)
        r = triplane(rp, rl, rb, src)
        worst.append(check(f"{kernel} scale {scale:g}", out[:, :F], r["out"], r["out_m"], k))
    print(f"{shape} {mode} {kernel}: worst err / (u M) per grid scale", " ".join(f"{w:.3g}" for w in worst))


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_gather_ragged_n_strided_output_and_sentinels(mode):
    """n = 1, 15, 16, 17, a wavefront / block tile +- 1; out_stride > app_dim with out_col > 0: the columns around the window keep their
    sentinel, rows past n are not written; n = 0 is a no-op"""
    lvl, gsz, planes, lines, basis = make_level("shipped", "fine", 0.1)
    half = MODES[mode][1]
    rp, rl, rb = ref_grids(planes, lines, basis, half)
    kernel = fwd_kernel("shipped", half)
    rs = np.random.RandomState(2)
    for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129):
        pts = rs.uniform(AABB[0], AABB[1], (n, 3)).astype(np.float32)
        out = torch.full((n + 3, 45), 1234.5, dtype=torch.float32, device="cuda")
        p = torch.tensor(pts, device="cuda")
        L.check(L.lib().evd_voxel_sample_prec(lvl.handle, L.PREC[mode], L.ptr(p), n, C.c_void_p(out.data_ptr()), 45, 7, L.stream_ptr()), "sample")
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[:, :7] == 1234.5).all() and (o[:, 7 + F:] == 1234.5).all() and (o[n:] == 1234.5).all(), n
        r = triplane(rp, rl, rb, src_indices(pts, AABB, gsz)[0])
        check(f"{kernel} n={n}", o[:n, 7:7 + F], r["out"], r["out_m"], fwd_bound(kernel, 96))
    out = torch.full((4, F), 1234.5, dtype=torch.float32, device="cuda")
    p = torch.zeros((1, 3), dtype=torch.float32, device="cuda")
    L.check(L.lib().evd_voxel_sample_prec(lvl.handle, L.PREC[mode], L.ptr(p), 0, C.c_void_p(out.data_ptr()), F, 0, L.stream_ptr()), "sample n=0")
    torch.cuda.synchronize()
    assert (out.cpu() == 1234.5).all()


# ---- backward ----------------------------------------------------------------------------------------------------------------------
BWD_ENTRIES = [("bwd", "f32"), ("bwd_ws", "f32")] + [("bwd_prec", m) for m in MODES]
BWD_CASES = []
for s in SHAPES:
    for e, m in BWD_ENTRIES:
        for dpts in (True, False):
            half = MODES[m][1] and e == "bwd_prec"
            BWD_CASES.append((s, e, m, dpts, bwd_kernel(s, e, half, dpts)))


def bwd_half(kernel, entry, mode):
    """the backward's re-gather reads the float16 copies only in the wavefront form, in a mode whose forward read them"""
    return entry == "bwd_prec" and MODES[mode][1] and kernel.startswith("k_voxel_sample_bwd_w")


def check_bwd(tag, kernel, r, gp, gl, gb, dp, n, ct, src=None):
    kd = 12 + SPLIT / U + 2 * F             # d coef: split-float16 product over F, or a float32 chain of F
    w = {}
    for i in range(3):
        w[f"plane{i}"] = check(f"{tag} d plane {i}", gp[i], r["d_plane"][i], r["d_plane_m"][i], kd + r["d_plane_cnt"][i].cpu() + 2)
        fixed = None
        if "k_scatter_lines" in kernel:
            fixed = r["d_line_cnt"][i].cpu() * 2.0 ** -48 * r["line_row_max"] * torch.ones_like(r["d_line"][i].cpu())
        w[f"line{i}"] = check(f"{tag} d line {i}", gl[i], r["d_line"][i], r["d_line_m"][i], kd + r["d_line_cnt"][i].cpu() + 4, fixed)
    if gb is not None:
        w["basis"] = check(f"{tag} d basis", gb, r["d_basis"], r["d_basis_m"], 12 + n / 16 + 64)
    if dp is not None:
        w["pts"] = check(f"{tag} d pts", dp[:n], r["d_pts"], r["d_pts_m"], kd + 3 * ct + 16, rows=None if src is None else [s.tolist() for s in src])
    return w


def d_out_rows(rs, n):
    """d out with a dynamic range across samples (rows at 2^-40 .. 1) and a realistic one within a row (2^-8 .. 1)"""
    return rs.normal(size=(n, F)) * 2.0 ** rs.uniform(-40, 0, (n, 1)) * 2.0 ** rs.uniform(-8, 0, (n, F))


@pytest.mark.parametrize("shape,entry,mode,dpts,kernel", BWD_CASES, ids=[f"{s}-{e}-{m}-{'dpts' if d else 'nodpts'}-{k}" for s, e, m, d, k in BWD_CASES])
def test_scatter_matches_float64_reference(shape, entry, mode, dpts, kernel):
    kind = MODES[mode][0]
    half = bwd_half(kernel, entry, mode)
    ct = sum(SHAPES[shape])
    worst = {}
    for si, scale in enumerate(SCALES):
        lvl, gsz, planes, lines, basis = make_level(shape, kind, scale, seed=7 + si)
        pts = points(gsz, 21 + si, n_rand=320)
        n = pts.shape[0]
        rs = np.random.RandomState(31 + si)
        d_out = d_out_rows(rs, n).astype(np.float32)
        src, kp = src_indices(pts, AABB, gsz)
        # strided d out rows on one scale: d_stride > app_dim, d_col > 0
        ds, dc = (40, 5) if si == 1 else (F, 0)
        gp, gl, gb, dp = run_bwd(lvl, entry, mode, pts, d_out, ds, dc, dpts=dpts, basis_grad=si != 2, planes=planes, lines=lines, basis=basis)
        rp, rl, rb = ref_grids(planes, lines, basis, half)
        r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
        for key, v in check_bwd(f"{kernel} scale {scale:g}", kernel, r, gp, gl, gb, dp, n, ct, src).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"{shape} {entry} {mode} {kernel}: worst err / (u M):", " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("entry", ["bwd", "bwd_ws"])
def test_scatter_n_zero_is_a_no_op(entry):
    lvl, gsz, planes, lines, basis = make_level("shipped", "fine", 0.1)
    gp, gl, gb, dp = run_bwd(lvl, entry, "f32", np.zeros((0, 3), np.float32), np.zeros((0, F), np.float32), planes=planes, lines=lines, basis=basis)
    assert all(float(t.abs().sum()) == 0 for t in gp + gl + [gb])
    assert torch.isnan(dp).all()          # the (1, 3) stand-in buffer: not written


@pytest.mark.parametrize("shape,entry,mode", [("shipped", "bwd_ws", "f32"), ("shipped", "bwd_prec", "f16"), ("shipped", "bwd", "f32"),
                                              ("ct128", "bwd_ws", "f32"), ("c12", "bwd_ws", "f32")])
def test_scatter_non_finite_d_out_reaches_every_gradient(shape, entry, mode):
    """+inf and NaN in one in-box row: the plane, line and basis gradients that row reaches are non-finite, the others finite and
    within their bounds (the line scatter's fixed point has no scale for a non-finite row and falls back to float atomics)"""
    kind = MODES[mode][0]
    lvl, gsz, planes, lines, basis = make_level(shape, kind, 0.1)
    kernel = bwd_kernel(shape, entry, MODES[mode][1] and entry == "bwd_prec", True)
    rs = np.random.RandomState(4)
    n = 200
    pts = rs.uniform(np.array(AABB[0]) * 0.9, np.array(AABB[1]) * 0.9, (n, 3)).astype(np.float32)
    d_out = rs.normal(size=(n, F)).astype(np.float32)
    d_out[5, 3], d_out[5, 9] = np.inf, np.nan
    gp, gl, gb, dp = run_bwd(lvl, entry, mode, pts, d_out, planes=planes, lines=lines, basis=basis)
    half = bwd_half(kernel, entry, mode)
    rp, rl, rb = ref_grids(planes, lines, basis, half)
    src, kp = src_indices(pts, AABB, gsz)
    r = triplane(rp, rl, rb, src, kpts=kp, d_out=d_out.astype(np.float64))
    assert not torch.isfinite(r["d_basis"]).all() and not torch.isfinite(r["d_line"][0]).all()
    check_bwd(kernel, kernel, r, gp, gl, gb, dp, n, sum(SHAPES[shape]))


# ---- the float16 copies ------------------------------------------------------------------------------------------------------------
def _boundary_1e5(sd):
    out = {}
    for i in range(3):
        p = np.array(sd[f"app_plane.{i}"], np.float32)
        p[..., 0, :], p[..., -1, :], p[..., :, 0], p[..., :, -1] = 1e5, -1e5, 1e5, -1e5
        l = np.array(sd[f"app_line.{i}"], np.float32)
        l[:, :, 0], l[:, :, -1] = 1e5, -1e5
        out[f"app_plane.{i}"], out[f"app_line.{i}"] = p, l
    return out


@pytest.mark.parametrize("shape", ["shipped", "ct80", "c12"])
def test_boundary_values_above_float16_range_give_zero_outside_the_box(shape):
    """boundary cells at +-1e5 (beyond float16): points outside the box read them through clamped taps with weight 0 -- exactly 0 in
    every mode; inside, the half modes see the saturated copy (+-65504) and stay finite and within their bound"""
    rs = np.random.RandomState(8)
    for kind in ("fine", "coarse"):
        lvl, gsz, planes, lines, basis = make_level(shape, kind, 0.1, grids=_boundary_1e5)
        lo, hi = np.array(AABB[0]), np.array(AABB[1])
        far = []
        for a in range(3):
            for off in (-0.3, 1.3, -5.0, 6.0):
                p = rs.uniform(lo, hi, (4, 3))
                p[:, a] = lo[a] + off * (hi[a] - lo[a])
                far.append(p)
        far = np.concatenate(far).astype(np.float32)
        inside = points(gsz, 9)
        for mode in (None, "f32", "f16x3", "f16", "bf16", "f16c"):
            out = run_fwd(lvl, mode, far)
            assert (out[:, :F] == 0).all(), (kind, mode)
            half = mode in ("f16", "bf16") or (mode == "f16c" and kind == "fine")
            kernel = fwd_kernel(shape, half)
            o = run_fwd(lvl, mode, inside)
            rp, rl, rb = ref_grids(planes, lines, basis, half)
            r = triplane(rp, rl, rb, src_indices(inside, AABB, gsz)[0])
            check(f"{kernel} {mode} 1e5 boundary", o[:, :F], r["out"], r["out_m"], fwd_bound(kernel, sum(SHAPES[shape])))


def test_device_float16_copy_equals_the_host_copy():
    """evd_voxel_load_grids (the device copy after each optimizer step) and evd_voxel_create (the host copy) make the same float16 grids:
    bit-identical features in every half mode, also for values beyond float16's range"""
    a, gsz, planes, lines, basis = make_level("shipped", "fine", 0.1, seed=12, grids=_boundary_1e5)
    b = make_level("shipped", "fine", 2.0, seed=13)[0]
    b.load_grids([torch.tensor(t, device="cuda") for t in planes + lines + [basis]])
    pts = points(gsz, 14)
    for mode in ("f16", "bf16", "f16c", "f32"):
        assert torch.equal(run_fwd(a, mode, pts), run_fwd(b, mode, pts)), mode


def test_f16c_reads_float32_grids_on_the_coarse_level_and_float16_on_the_fine():
    """grids_half_for: in f16c the coarse level's gather equals f32 bit for bit, the fine level's equals f16 bit for bit"""
    for kind, twin in (("coarse", "f32"), ("fine", "f16")):
        lvl, gsz, *_ = make_level("shipped", kind, 0.1)
        pts = points(gsz, 15)
        assert torch.equal(run_fwd(lvl, "f16c", pts), run_fwd(lvl, twin, pts)), kind


# ---- the shipped fine size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16", "f16x3"])
def test_gather_at_the_shipped_fine_size_uses_the_largest_tap_offsets(mode):
    """586 x 586 x 390 (fine_n_voxels 134217984): points on the far corner, the far faces and one ulp inside them, where the 32-bit tap
    offsets are largest; reference in float64 on the device"""
    nvox = 134217984
    gsz = W.pdrf_grid_size(AABB[0], AABB[1], nvox)
    assert gsz == [586, 586, 390]
    rs = np.random.RandomState(16)
    nc = (64, 16, 16)
    sd = {}
    for i, (m0, m1) in enumerate([[0, 1], [0, 2], [1, 2]]):
        sd[f"app_plane.{i}"] = (0.1 * rs.standard_normal((1, nc[i], gsz[m1], gsz[m0]))).astype(np.float32)
        sd[f"app_line.{i}"] = (0.1 * rs.standard_normal((1, nc[i], gsz[[2, 1, 0][i]], 1))).astype(np.float32)
    net = dict(input_ch=127, hidden_dim=256, geo_feat_dim=128)
    base = W.make_pdrf_state_dict(17, [4, 4, 4], app_n_comp=nc, **net)
    base.update(sd)
    basis = (rs.standard_normal((F, 96)) * 0.1).astype(np.float32)
    base["basis_mat.weight"] = basis
    lvl = VoxelNeRFBase(base, "", AABB, app_n_comp=nc, n_voxels=nvox, rgb_activate="none", **net)
    want = []
    for c in range(8):                      # near the far corner: every axis on the far face or half a cell inside it
        want.append([float(gsz[a] - 1) if (c >> a) & 1 else float(gsz[a] - 1) - 0.5 for a in range(3)])
    for a in range(3):                      # one axis on the far face / one ulp inside it / the last interior integer, the others random near it
        for t in (float(gsz[a] - 1), float(np.nextafter(np.float32(gsz[a] - 1), np.float32(0))), float(gsz[a] - 2)):
            w = [np.nan, np.nan, np.nan]
            w[a] = t
            want.append(w)
    want = np.array(want * 8)
    pts = index_points(AABB, gsz, want, rs)
    lo, hi = np.array(AABB[0], np.float32), np.array(AABB[1], np.float32)
    pts = np.where(np.isnan(want), hi - (hi - lo) * rs.uniform(0, 0.01, pts.shape), pts).astype(np.float32)
    half = mode == "f16"
    kernel = fwd_kernel("shipped", half)
    out = run_fwd(lvl, mode, pts)
    src, _ = src_indices(pts, AABB, gsz)
    dev = lambda t: torch.tensor(np.ascontiguousarray(t), device="cuda")
    cv = (lambda t: f16_copy(dev(t))) if half else (lambda t: dev(t).double())
    planes = [cv(np.asarray(sd[f"app_plane.{i}"])[0].transpose(1, 2, 0)) for i in range(3)]
    lines = [cv(np.asarray(sd[f"app_line.{i}"])[0, :, :, 0].T) for i in range(3)]
    del sd, base
    r = triplane(planes, lines, dev(basis).double(), src)
    worst = check(f"{kernel} 586x586x390", out[:, :F], r["out"], r["out_m"], fwd_bound(kernel, 96))
    print(f"fine size {mode} {kernel}: worst err / (u M) {worst:.3g}")
