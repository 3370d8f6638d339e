"""float64 reference of the tri-plane gather (VoxelNeRFBase.sample / compute_appfeature, voxnerf.py:132-151,203-208) and of its
backward, with a per-element magnitude for every output.  Test infrastructure only.

The source coordinates are the one part kept in float32, computed exactly as the reference computes them: xyz = (p - aabb_min) *
invaabbSize - 1 (voxnerf.py:205, float32 tensors), then ATen's align-corners unnormalise ((c + 1) / 2) * (size - 1).  At a fine grid
one float32 ulp of the source index is ~6e-5 cells, far more than any bound the kernels are held to, so the kernel and the reference
must agree on that index bit for bit.  Everything after it -- taps, weights, products, the basis product -- is float64.

Grids are in the library's channel-last layout: plane i [grid[m1], grid[m0], C_i], line i [grid[v], C_i], basis [app_dim, sum C].
The magnitude of an output is the same expression evaluated on absolute values (|B|, |plane|, |line|, |d out|, |d weight|): every
rounding error of a kernel that evaluates the expression in some order is bounded by a multiple of it."""
import numpy as np
import torch

MAT, VEC = [[0, 1], [0, 2], [1, 2]], [2, 1, 0]
F16_MAX = 65504.0


def source_index32(pts, aabb):
    """pts float32 [n, 3], aabb (lo[3], hi[3]) -> xyz float32 [n, 3] (voxnerf.py:205) with invaabbSize as the reference builds it
    (2.0 / (hi - lo) in float32, voxnerf.py:91)"""
    lo, hi = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
    inv = (np.float32(2.0) / (hi - lo)).astype(np.float32)
    p = np.asarray(pts, np.float32)
    return ((p - lo) * inv - np.float32(1.0)).astype(np.float32), inv


def unnorm32(c, size):
    """ATen grid_sampler_unnormalize, align_corners=True, in float32: ((c + 1) / 2) * (size - 1)"""
    c = np.asarray(c, np.float32)
    return (((c + np.float32(1.0)) / np.float32(2.0)) * np.float32(size - 1)).astype(np.float32)


def src_indices(pts, aabb, grid):
    """float32 source index per point axis [n, 3] (axis a is unnormalised with grid[a] wherever it is read) and d index / d point [3]
    (float64: the exact derivative of the float32 pipeline's real-number form with the float32 invaabbSize)"""
    xyz, inv = source_index32(pts, aabb)
    s = np.stack([unnorm32(xyz[:, a], grid[a]) for a in range(3)], 1)
    k = np.array([0.5 * (grid[a] - 1) * float(inv[a]) for a in range(3)])
    return s, k


def f16_copy(x):
    """the float16 copy a half-precision mode gathers: round to nearest, saturated to the finite range (NaN stays NaN)"""
    x = torch.as_tensor(x)
    return torch.where(x.isnan(), x, x.clamp(-F16_MAX, F16_MAX)).to(torch.float16).to(torch.float64)


def _lin(idx_f, size):
    """floor tap, weight of the upper tap, validity of both taps, clamped indices"""
    i0 = torch.floor(idx_f)
    w = idx_f - i0                       # exact
    i0l = i0.clamp(-2, size).long()      # far points: both taps are outside whatever the clamp
    i1l = i0l + 1
    v0, v1 = (i0l >= 0) & (i0l < size), (i1l >= 0) & (i1l < size)
    return w, v0, v1, i0l.clamp(0, size - 1), i1l.clamp(0, size - 1)


def _comp(plane, line, sx, sy, sl):
    """one component: pv, lv, d pv / d sx, d pv / d sy, d lv / d sl [n, C] and their magnitudes, plus the tap tables"""
    H, Wd, C = plane.shape
    Lp = line.shape[0]
    wx, vx0, vx1, x0, x1 = _lin(sx, Wd)
    wy, vy0, vy1, y0, y1 = _lin(sy, H)
    ex, ey = 1 - wx, 1 - wy
    zero = torch.zeros((), dtype=torch.float64, device=plane.device)
    taps = [(x0, y0, vx0 & vy0, ex * ey, -ey, -ex), (x1, y0, vx1 & vy0, wx * ey, ey, -wx),
            (x0, y1, vx0 & vy1, ex * wy, -wy, ex), (x1, y1, vx1 & vy1, wx * wy, wy, wx)]
    pv = pm = dx = dxm = dy = dym = 0
    ptab = []
    for xi, yi, ok, w, gx, gy in taps:
        v = plane[yi, xi]                                           # [n, C]
        okc = ok[:, None]
        v = torch.where(okc, v, zero)                               # zero padding: the outside tap is a zero VALUE (ATen)
        a = v.abs()
        pv = pv + w[:, None] * v
        pm = pm + w[:, None] * a
        dx, dxm = dx + gx[:, None] * v, dxm + gx.abs()[:, None] * a
        dy, dym = dy + gy[:, None] * v, dym + gy.abs()[:, None] * a
        ptab.append((yi * Wd + xi, torch.where(ok, w, zero)))
    wl, vl0, vl1, l0, l1 = _lin(sl, Lp)
    el = 1 - wl
    u0 = torch.where(vl0[:, None], line[l0], zero)
    u1 = torch.where(vl1[:, None], line[l1], zero)
    lv = el[:, None] * u0 + wl[:, None] * u1
    lm = el[:, None] * u0.abs() + wl[:, None] * u1.abs()
    dl, dlm = u1 - u0, u1.abs() + u0.abs()
    ltab = [(l0, torch.where(vl0, el, zero)), (l1, torch.where(vl1, wl, zero))]
    return dict(pv=pv, pm=pm, dx=dx, dxm=dxm, dy=dy, dym=dym, lv=lv, lm=lm, dl=dl, dlm=dlm, ptab=ptab, ltab=ltab)


def triplane(planes, lines, basis, src, kpts=None, d_out=None):
    """float64 forward (and, with d_out [n, F], backward) of the gather at float32 source indices src [n, 3].
    Returns a dict: out, out_m; with d_out: d_plane[i], d_plane_m[i], d_plane_cnt[i], d_line[i], d_line_m[i], d_line_cnt[i] (contributions per cell),
    line_row_max (max |d coef x pv| over the batch: the scale of the line scatter's fixed point), d_basis, d_basis_m, d_pts, d_pts_m."""
    dev = planes[0].device
    f64 = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float64)
    planes, lines, basis = [f64(p) for p in planes], [f64(l) for l in lines], f64(basis)
    s = f64(src)
    comps = [_comp(planes[i], lines[i], s[:, MAT[i][0]], s[:, MAT[i][1]], s[:, VEC[i]]) for i in range(3)]
    coef = torch.cat([c["pv"] * c["lv"] for c in comps], 1)
    coef_m = torch.cat([c["pm"] * c["lm"] for c in comps], 1)
    r = dict(out=coef @ basis.T, out_m=coef_m @ basis.abs().T, coef=coef, coef_m=coef_m)
    if d_out is None:
        return r
    g = f64(d_out)
    dco, dcom = g @ basis, g.abs() @ basis.abs()
    r["d_basis"], r["d_basis_m"] = g.T @ coef, g.abs().T @ coef_m
    off = 0
    kp = f64(kpts) if kpts is not None else torch.ones(3, dtype=torch.float64, device=dev)
    dp, dpm = torch.zeros_like(s), torch.zeros_like(s)
    r["d_plane"], r["d_plane_m"], r["d_plane_cnt"], r["d_line"], r["d_line_m"], r["d_line_cnt"] = [], [], [], [], [], []
    rmax = 0.0
    for i, c in enumerate(comps):
        C = planes[i].shape[2]
        d, dm = dco[:, off:off + C], dcom[:, off:off + C]
        off += C
        H, Wd = planes[i].shape[:2]
        gp, gpm = torch.zeros((H * Wd, C), dtype=torch.float64, device=dev), torch.zeros((H * Wd, C), dtype=torch.float64, device=dev)
        pcnt = torch.zeros((H * Wd,), dtype=torch.float64, device=dev)
        for idx, w in c["ptab"]:
            gp.index_add_(0, idx, w[:, None] * d * c["lv"])
            gpm.index_add_(0, idx, w[:, None] * dm * c["lm"])
            pcnt.index_add_(0, idx, (w != 0).double())
        Lp = lines[i].shape[0]
        gl, glm = torch.zeros((Lp, C), dtype=torch.float64, device=dev), torch.zeros((Lp, C), dtype=torch.float64, device=dev)
        cnt = torch.zeros((Lp,), dtype=torch.float64, device=dev)
        for idx, w in c["ltab"]:
            gl.index_add_(0, idx, w[:, None] * d * c["pv"])
            glm.index_add_(0, idx, w[:, None] * dm * c["pm"])
            cnt.index_add_(0, idx, (w != 0).double())
        rmax = max(rmax, float((dm * c["pm"]).max()) if d.numel() else 0.0)
        r["d_plane"].append(gp.view(H, Wd, C))
        r["d_plane_m"].append(gpm.view(H, Wd, C))
        r["d_plane_cnt"].append(pcnt.view(H, Wd, 1))
        r["d_line"].append(gl)
        r["d_line_m"].append(glm)
        r["d_line_cnt"].append(cnt[:, None])
        a0, a1, al = MAT[i][0], MAT[i][1], VEC[i]
        dp[:, a0] += (d * c["dx"] * c["lv"]).sum(1)
        dp[:, a1] += (d * c["dy"] * c["lv"]).sum(1)
        dp[:, al] += (d * c["pv"] * c["dl"]).sum(1)
        dpm[:, a0] += (dm * c["dxm"] * c["lm"]).sum(1)
        dpm[:, a1] += (dm * c["dym"] * c["lm"]).sum(1)
        dpm[:, al] += (dm * c["pm"] * c["dlm"]).sum(1)
    r["d_pts"], r["d_pts_m"] = dp * kp, dpm * kp.abs()
    r["line_row_max"] = rmax
    return r


def to_channel_last(sd, prefix=""):
    """reference state-dict layouts ([1,C,H,W] planes, [1,C,L,1] lines) -> the library's channel-last grids (float32 numpy)"""
    planes = [np.ascontiguousarray(np.asarray(sd[f"{prefix}app_plane.{i}"], np.float32)[0].transpose(1, 2, 0)) for i in range(3)]
    lines = [np.ascontiguousarray(np.asarray(sd[f"{prefix}app_line.{i}"], np.float32)[0, :, :, 0].T) for i in range(3)]
    return planes, lines, np.asarray(sd[f"{prefix}basis_mat.weight"], np.float32)


def index_points(aabb, grid, want, rs):
    """points whose float32 source index on every axis is EXACTLY a wanted value (want [n, 3] float64, e.g. an integer, 0, size - 1,
    or one float32 ulp next to one): start from the real-number inverse and step the float32 point with nextafter until the float32
    pipeline gives the wanted index; axes whose wanted value is NaN get a uniform random in-box coordinate."""
    lo, hi = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
    _, inv = source_index32(np.zeros((1, 3), np.float32), aabb)
    n = want.shape[0]
    pts = np.empty((n, 3), np.float32)
    for a in range(3):
        tgt = want[:, a]
        rnd = np.isnan(tgt)
        p = np.where(rnd, rs.uniform(lo[a], hi[a], n), lo[a] + (tgt / (grid[a] - 1)) * (hi[a] - lo[a])).astype(np.float32)
        for _ in range(64):
            s = unnorm32((p - lo[a]) * inv[a] - np.float32(1.0), grid[a]).astype(np.float64)
            bad = ~rnd & (s != tgt)
            if not bad.any():
                break
            p = np.where(bad, np.nextafter(p, np.where(s < tgt, np.float32(np.inf), np.float32(-np.inf))), p).astype(np.float32)
        pts[:, a] = p        # an index the float32 pipeline steps over: the nearest one reached (the caller checks what it needs)
    return pts


def edge_points(aabb, grid, rs, n_rand=64):
    """the gather's edge cases: exact box faces (index 0 and size - 1), exact interior integers (those the float32 pipeline can land
    on), one float32 ulp either side of each, points just and far outside, mixed per axis with random coordinates"""
    grid = [int(g) for g in grid]
    rows = []
    for a in range(3):
        G = grid[a]
        want = np.full((G, 3), np.nan)
        want[:, a] = np.arange(G)
        src, _ = src_indices(index_points(aabb, grid, want, rs), aabb, grid)
        inner = [t for t in range(1, G - 1) if src[t, a] == t]
        for t in [0.0, float(G - 1)] + [float(t) for t in inner[:: max(1, len(inner) // 3)][:3]]:
            for d in (0, -1, 1):
                v = np.float32(t)
                if d:
                    v = np.nextafter(v, np.float32(np.inf) if d > 0 else np.float32(-np.inf))
                w = np.full(3, np.nan)
                w[a] = float(v)
                rows.append(w)
    # corners: every axis on a face
    for c in range(8):
        rows.append(np.array([0.0 if not (c >> a) & 1 else float(grid[a] - 1) for a in range(3)]))
    want = np.array(rows)
    pts = index_points(aabb, grid, want, rs)
    lo, hi = np.asarray(aabb[0], np.float64), np.asarray(aabb[1], np.float64)
    ext = hi - lo
    out = [pts]
    # just outside (within one cell) and far outside on each axis, the others random
    for a in range(3):
        for off in (-0.5 / (grid[a] - 1), 1 + 0.5 / (grid[a] - 1), -40.0, 41.0, -1e6):        # half a cell out, far out (box extents)
            p = rs.uniform(lo, hi, (2, 3))
            p[:, a] = lo[a] + off * ext[a]
            out.append(p.astype(np.float32))
    out.append(rs.uniform(lo, hi, (n_rand, 3)).astype(np.float32))
    return np.concatenate(out).astype(np.float32)
