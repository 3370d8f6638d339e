"""The tile walk of the training backward's persistent kernels, restated on the CPU: which workgroup processes which sample tiles, the
cases of tests/test_gpu_bwd_walk.py with their inputs, and the float64 autograd references of the three networks.

Stores are tiled in groups of 8 tiles of 32 samples (train_tiles / vox_tiles / awp_tiles).  The cases use nsamp = 256 k - 83: the last
group then holds 5 full tiles, one ragged tile of 13 samples and 2 tiles that are all padding.

Two walks exist:
  * k_wgrad / k_wgrad_split / k_wgrad_dgrad (nerf_bwd_wgrad.h, nerf_bwd_fused.h): min(tiles, blocks) workgroups, workgroup b takes
    tiles b, b + grid, b + 2 grid, ... one per iteration (`walk_split`).  blocks = the EVD_BWD_OVERLAP workgroup count with a side
    stream, 256 without (`nerf_blocks`, `level_blocks`).
  * k_voxel_bwd_fused64 / k_awp_bwd_fused (voxel_bwd_fused64.h, awp_bwd_fused.h): min(cdiv(tiles, 4), 256) workgroups of 4 wavefronts,
    wavefront w of workgroup b takes tiles 4 b + w, 4 b + w + 4 grid, ... (`wave_split`: per workgroup, per pass, the tiles of its
    wavefronts).

Inputs.  d raw is a normal draw times a per-sample log-uniform factor exp(U(-4, 0)), as in tests/test_gpu_train.py.  The parameter
gradients are linear in d raw, so a walk that drops a tile or counts it twice gives float64 autograd with that tile's d raw scaled by 0
or 2: tests/test_bwd_walk_ref.py asserts that every such fault moves every parameter gradient by 10 x the bound the GPU test holds it
to.  One tile among hundreds carries a few per cent of a gradient, less than 10 x the bfloat16 bound; so within the tiles a case SWEEPS
(`Case.sweep`) the factors are multiplied by one number per tile that gives each of them the share SWEEP_SHARE of sum factor^2 (all
sample-holding tiles swept: equal shares).  The other tiles keep their draw.  The price: on the production rows one tile of 200 or 264
then dominates the float64 comparison, and a fault confined to ANOTHER workgroup's second tile (under 1 % of sum factor^2) would stay
within the bf16 bound; the small rows, where every workgroup's tiles carry a like share, are what holds those.  Test infrastructure only."""
import math
from collections import namedtuple

import numpy as np
import torch

from evdeblurnerf_amd import weights as W
from nerf_generic_ref import TAU, TIE_CAP  # noqa: F401  (the f16x3 mode's ReLU ties: the project's threshold and cap)
from torch_restatement import TorchNerf, TorchVoxLevel, embed

AABB = ((-1.5, -1.5, -1.0), (1.5, 1.5, 1.0))
SWEEP_SHARE = 0.2           # of sum factor^2 per swept tile: sqrt(0.2) = 0.45 of an incoherent gradient sum, above 10 x 3e-2


def nsamp_of(k):
    return 256 * k - 83


def tiles_of(nsamp):
    return -(-nsamp // 256) * 8


def tile_samples(nsamp, t):
    """samples that tile t holds: 32, a ragged count, or 0 (all padding)"""
    return max(0, min(32, nsamp - 32 * t))


def nerf_blocks(overlap):
    """BwdPlan::wgrad_blocks of evd_nerf_mlp_backward; overlap: the value of EVD_BWD_OVERLAP or None (unset)"""
    want = 192 if overlap is None else int(overlap)
    return 256 if want <= 0 else min(want, 256)


def level_blocks(overlap, overlap_voxel):
    """... of evd_voxel_mlp_backward: the side stream (and its workgroup count) only with EVD_BWD_OVERLAP_VOXEL"""
    return nerf_blocks(overlap) if overlap_voxel else 256


def walk_split(tiles, blocks):
    """tile list of every workgroup of a grid-stride wgrad / fused launch"""
    grid = min(tiles, blocks)
    return [list(range(b, tiles, grid)) for b in range(grid)]


def wave_split(tiles, cap=256):
    """per workgroup, per pass: the tiles of its (up to 4) wavefronts in k_voxel_bwd_fused64 / k_awp_bwd_fused"""
    grid = min(-(-tiles // 4), cap)
    out = []
    for b in range(grid):
        passes, base = [], 4 * b
        while base < tiles:
            passes.append([t for t in range(base, base + 4) if t < tiles])
            base += 4 * grid
        out.append(passes)
    return out


def split_summary(counts):
    """[2, 2, 1, 1, 1] -> '2 x 2, 3 x 1' (workgroups x tiles or passes)"""
    runs = {}
    for c in counts:
        runs[c] = runs.get(c, 0) + 1
    return ", ".join(f"{n} x {c}" for c, n in sorted(runs.items(), reverse=True))


def smallest_wave_cases(cap=256):
    """the smallest nsamp = 256 k - 83 for which (i) some but not all workgroups make a second pass and one of them has fewer than four
    live wavefronts (tiles that hold samples) in it, (ii) every workgroup makes at least three passes"""
    found = {}
    k = 1
    while len(found) < 2:
        n = nsamp_of(k)
        sp = wave_split(tiles_of(n), cap)
        npass = [len(p) for p in sp]
        second = [p[1] for p in sp if len(p) > 1]
        if "i" not in found and 0 < len(second) < len(sp) and any(sum(tile_samples(n, t) > 0 for t in p) < 4 for p in second):
            found["i"] = n
        if "ii" not in found and min(npass) >= 3:
            found["ii"] = n
        k += 1
    return found["i"], found["ii"]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# (EVD_BWD_OVERLAP, nsamp of the NeRF trunk, nsamp of the fine level) -- the table of the walk's lengths; None: the variable unset.
# The fine level runs with EVD_BWD_OVERLAP_VOXEL=1 on the small rows (the NeRF trunk's grid) and with its shipped 256 workgroups on the
# two production rows.
ROWS = [("1", 173, 173), ("3", 173, 173), ("5", 429, 429), ("7", 173, 173), (None, 6317, 8365), ("0", 8365, 8365)]
SMALL_ROWS = ("1", "3", "5", "7")
NERF_PRECS = ("f16", "bf16", "f16x3")
LEVEL_PRECS = ("f16", "bf16")
TOL = {"f16": 4e-3, "bf16": 3e-2, "f16x3": 5e-6}         # tests/test_gpu_train.py, tests/test_gpu_train_f32grade.py
TOL_AWP = {"f16": 4e-3, "bf16": 3e-2}                    # tests/test_gpu_awp.py
CROSS_GRID_TOL = 1e-5                                    # tests/test_gpu_bwd_fusion.py: float32 partial sums in another order


def tol(net, prec, name):
    """the bound of one gradient tensor: parameter and per-sample gradients of a mode alike (f16x3: 5e-6 for d_pts / d_dirs too)"""
    return TOL_AWP[prec] if net == "awp" else TOL[prec]


Case = namedtuple("Case", "name net nsamp blocks sweep")     # sweep: the tiles whose d raw carries SWEEP_SHARE (the CPU test scales them)


def _sweep_walk(nsamp, blocks):
    """the tiles of one multi-tile workgroup: the one with the most sample-holding tiles, the ragged tile's on a draw; on the production
    grids (two-tile workgroups) its second tile"""
    tiles = tiles_of(nsamp)
    sp = walk_split(tiles, blocks)
    ragged = (nsamp - 1) // 32
    best = max(sp, key=lambda ts: (len(ts) > 1, sum(tile_samples(nsamp, t) > 0 for t in ts), ragged in ts))
    live = [t for t in best if tile_samples(nsamp, t) > 0]
    return live if len(sp) < 64 else live[1:2]


def walk_cases(overlap):
    """the NeRF and fine-level cases of one EVD_BWD_OVERLAP row"""
    row = next(r for r in ROWS if r[0] == overlap)
    small = overlap in SMALL_ROWS
    nb, lb = nerf_blocks(overlap), level_blocks(overlap, small)
    return [Case(f"nerf{row[1]}", "nerf", row[1], nb, _sweep_walk(row[1], nb)), Case(f"fine{row[2]}", "fine", row[2], lb, _sweep_walk(row[2], lb))]


def wave_cases():
    """(b): the 64-wide level and the AWP embedding at the two smallest sample counts of `smallest_wave_cases`; swept: one second-pass
    tile of a full wavefront set and the ragged tile"""
    out = []
    for n in smallest_wave_cases():
        tiles = tiles_of(n)
        sweep = [4 * min(-(-tiles // 4), 256), (n - 1) // 32]
        out += [Case(f"coarse{n}", "coarse", n, 256, sweep), Case(f"awp{n}", "awp", n, 256, sweep)]
    return out


def reduced_wave_cases(cap=3):
    """the same two split shapes with `cap` workgroups instead of 256 (the CPU test's reduced sample sets)"""
    out = []
    for n in smallest_wave_cases(cap):
        sweep = [4 * min(-(-tiles_of(n) // 4), cap), (n - 1) // 32]
        out += [Case(f"coarse{n}", "coarse", n, cap, sweep), Case(f"awp{n}", "awp", n, cap, sweep)]
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def sample_factors(nsamp, sweep, rs):
    """per-sample log-uniform factor exp(U(-4, 0)); the swept tiles rescaled to their share of sum factor^2 (module docstring)"""
    f = np.exp(rs.uniform(-4, 0, nsamp))
    tile = np.arange(nsamp) // 32
    swept = np.isin(tile, sweep)
    if not len(sweep):
        return f
    e_rest = float((f[~swept] ** 2).sum())
    k = len(sweep)
    target = SWEEP_SHARE * e_rest / (1 - k * SWEEP_SHARE) if (e_rest > 0 and k * SWEEP_SHARE < 0.95) else 1.0
    for t in sweep:
        sel = tile == t
        f[sel] *= math.sqrt(target / float((f[sel] ** 2).sum()))
    return f


# Seeds.  A bias or the one-row alpha_linear sums its samples' gradients coherently, so what share of it one tile carries is a matter
# of the draw: for each case of the CPU test the first seed (counted from 1) at which every swept tile moves every parameter gradient by
# 10 x the bf16 bound in the float64 reference alone -- (net, nsamp, swept tiles) -> seed; every other case: 1
SEEDS = {("nerf", 173, (0, 1, 2, 3, 4, 5)): 90, ("nerf", 6317, (197,)): 3, ("fine", 429, (3, 8, 13)): 3, ("coarse", 429, (12, 13)): 7,
         ("coarse", 1197, (12, 37)): 7}


def case_inputs(case, seed=None):
    """every input of a case as float32 numpy arrays (one sample per ray: the walk is over sample tiles)"""
    n = case.nsamp
    rs = np.random.RandomState((SEEDS.get((case.net, n, tuple(case.sweep)), 1) if seed is None else seed) * 1000003 + n)
    d = rs.normal(size=(n, 3))
    vd = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    inp = {}
    if case.net == "nerf":
        rb = np.zeros((n, 11), np.float32)
        rb[:, 0:3] = rs.uniform(-0.5, 0.5, (n, 3))
        rb[:, 3:6], rb[:, 6], rb[:, 7], rb[:, 8:11] = vd, 0.0, 1.0, vd
        z = rs.uniform(0.2, 2.0, (n, 1)).astype(np.float32)
        inp.update(rb=rb, z=z, pts=(rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).astype(np.float32))
        gscale = 1e-4
    elif case.net in ("fine", "coarse"):
        FT, G = (64, 128) if case.net == "fine" else (32, 15)
        inp.update(pts=rs.uniform(-1, 1, (n, 1, 3)).astype(np.float32), vd=vd, fts=(0.3 * rs.normal(size=(n, 1, FT))).astype(np.float32))
        gscale = 1e-3
    else:
        inp.update(x=(rs.standard_normal((n, 128)) * 0.7).astype(np.float32))
        gscale = 1e-4
    f = sample_factors(n, case.sweep, rs)
    if case.net == "awp":
        inp["d_h"] = (rs.standard_normal((n, 64)) * gscale * f[:, None]).astype(np.float32)
    else:
        inp["d_raw"] = (rs.normal(size=(n, 1, 4)) * gscale * f[:, None, None]).astype(np.float32)
    if case.net == "fine":      # the gradient that arrives from the geo rows (the level's second output)
        inp["d_geo"] = (rs.normal(size=(n, 1, 128)) * 3e-4 * f[:, None, None]).astype(np.float32)
    return inp


def scale_tile(inp, t, s):
    """the inputs with every incoming gradient of tile t times s: what a walk that drops (0) or repeats (2) the tile computes"""
    out = dict(inp)
    for k in ("d_raw", "d_geo", "d_h"):
        if k in inp:
            a = inp[k].copy()
            a[32 * t:32 * t + 32] *= s
            out[k] = a
    return out


# ---- networks and float64 references ------------------------------------------------------------------------------------------------
def state_dict(net):
    if net == "nerf":
        return W.make_nerf_state_dict(22)
    if net == "awp":
        return W.make_awp_embed_state_dict(211)
    HD, G, FT, nvox = (256, 128, 64, 48 ** 3) if net == "fine" else (64, 15, 32, 24 ** 3)
    return W.make_pdrf_state_dict(71, W.pdrf_grid_size(AABB[0], AABB[1], nvox), input_ch=FT + 63, hidden_dim=HD, geo_feat_dim=G, add_bias_color=True)


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def reference(case, sd, inp, masks=None, rows=None):
    """float64 autograd of the restated network -> {tensor name: gradient}: every parameter and every input gradient the kernels form.
    masks: the kernel's own ReLU patterns (None: the network's own); rows: a slice of samples (gradients of a sample subset; the
    parameter gradients of disjoint subsets add up)"""
    sl = slice(None) if rows is None else rows
    out = {}
    if masks is not None:
        masks = {k: v[sl] for k, v in masks.items()} if isinstance(masks, dict) else [m[sl] for m in masks]
    if case.net == "nerf":
        net = TorchNerf(sd)
        p, v = _t64(inp["pts"][sl].reshape(-1, 3), True), _t64(inp["rb"][sl, 8:11], True)
        (net(p, v, masks=masks) * _t64(inp["d_raw"][sl].reshape(-1, 4))).sum().backward()
        out.update({k: net.p[k.replace(".", "_")].grad for k in sd})
        out["d_pts"], out["d_dirs"] = p.grad, v.grad
    elif case.net in ("fine", "coarse"):
        net = TorchVoxLevel(sd)
        p, v = _t64(inp["pts"][sl].reshape(-1, 3), True), _t64(inp["vd"][sl], True)
        f = _t64(inp["fts"][sl].reshape(p.shape[0], -1), True)
        raw, geo = net(p, v, f, masks=masks, want_geo=True)
        loss = (raw * _t64(inp["d_raw"][sl].reshape(-1, 4))).sum()
        if "d_geo" in inp:
            loss = loss + (geo * _t64(inp["d_geo"][sl].reshape(p.shape[0], -1))).sum()
        loss.backward()
        out.update({k: net.p[k.replace(".", "_")].grad for k in TorchVoxLevel.KEYS})
        out["d_pts"], out["d_dirs"], out["d_fts"] = p.grad, v.grad, f.grad
    else:
        ws = [_t64(sd[f"sample_feature_embed_layer.{l}.weight"], True) for l in range(4)]
        bs = [_t64(sd[f"sample_feature_embed_layer.{l}.bias"], True) for l in range(4)]
        x = _t64(inp["x"][sl], True)
        h = x
        for l in range(4):
            pre = h @ ws[l].t() + bs[l]
            h = pre * masks[l] if masks is not None else torch.relu(pre)
        (h * _t64(inp["d_h"][sl])).sum().backward()
        for l in range(4):
            out[f"w{l}"], out[f"b{l}"] = ws[l].grad, bs[l].grad
        out["d_geo_rows"] = x.grad
    return {k: g.detach().numpy() for k, g in out.items()}


def reference_chunked(case, sd, inp, masks=None, chunk=16384):
    """`reference` over chunks of samples: parameter gradients summed, input gradients concatenated"""
    n = case.nsamp
    if n <= chunk:
        return reference(case, sd, inp, masks)
    total = None
    for lo in range(0, n, chunk):
        part = reference(case, sd, inp, masks, rows=slice(lo, min(n, lo + chunk)))
        if total is None:
            total = {k: ([v] if k.startswith("d_") else v.copy()) for k, v in part.items()}
        else:
            for k, v in part.items():
                if k.startswith("d_"):
                    total[k].append(v)
                else:
                    total[k] += v
    return {k: (np.concatenate(v) if k.startswith("d_") else v) for k, v in total.items()}


def nerf_tie_samples(sd, inp, tau=TAU):
    """[n] bool: samples with a float64 pre-activation of the 8 x 256 network inside (-tau, tau) -- a unit that rounding decides in any
    float32-grade arithmetic (tests/test_gpu_nerf_generic_train.py)"""
    with torch.no_grad():
        p = {k: _t64(v) for k, v in sd.items()}
        lin = lambda name, x: x @ p[name + ".weight"].T + p[name + ".bias"]
        pe, ped = embed(_t64(inp["pts"].reshape(-1, 3)), 10), embed(_t64(inp["rb"][:, 8:11]), 4)
        h, tie = pe, torch.zeros(pe.shape[0], dtype=torch.bool)
        for l in range(8):
            pre = lin(f"pts_linears.{l}", h)
            tie |= (pre.abs() < tau).any(-1)
            h = torch.relu(pre)
            if l == 4:
                h = torch.cat([pe, h], -1)
        tie |= (lin("views_linears.0", torch.cat([lin("feature_linear", h), ped], -1)).abs() < tau).any(-1)
    return tie.numpy()


def is_param(name):
    return not name.startswith("d_")


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
