"""float64 references of the two per-ray steps a composite_feature level (kernel_type PBE, voxnerf.py:223-239) adds to the training
path, each with a first-order error bound per element, in units of u = 2^-24.  Test infrastructure only.

1. feat_composite_bwd: backward of fmap_c = sum_i w_i act(rows_ic), hand-written in the decomposition of k_composite_feat_bwd -- which is
   k_composite_rows_bwd's (composite_ref.py) with the three colours replaced by G geo channels:
     dot_i = sum_c g_fmap_c act(rows_ic)      one fma per channel, in channel order: sum |g_c| E_act + (G + 1) sum |g_c act|
     G_i   = dot_i + g_depth z_i + g_acc + g_w_i          E_dot + 5 M_i,  M_i = sum |g_c act| + |g_depth z_i| + |g_acc| + |g_w_i|
     suffix, d density, d sigma, d rays_d    as composite_ref.composite_bwd (form "bwd": SPL - 1 + 7 roundings along a row sum)
     d rows_ic = g_fmap_c w_i act'(rows_ic)  |g_c| (E_w |act'| + |w| E_act' + 2 |w act'|)
   The forward quantities and their bounds come from composite_ref._scan on cat([sigma, rows]).

2. color_rows: the per-ray colour network (cat([map, PE(dirs)]) -> Linear ReLU Linear ReLU Linear sigmoid) forward and backward.
     layer y_j = b_j + sum_i W_ji x_i        one fma per input, in input order: sum |W_ji| E_x_i + (n + 1) (|b_j| + sum |W_ji x_i|)
     PE(dirs)                                sinf / cosf of d 2^k, an exact product that the float64 evaluation shares: 4 |v| (2 ulp of
                                             the value, doubled)
     ReLU                                    passes the bound where y > 0.  A unit with |y| <= 4 u E_y may decide differently in float32:
                                             `unsure` marks such rays, from the float64 values alone
     sigmoid                                 composite_ref._act (code 2)
     d2 = g s (1 - s)                        from the float32 s: |g| (|1 - 2 s| E_s + 4 s (1 - s))
     d h = mask (W^T d)                      sum |W| E_d + (n + 1) sum |W d|,  n the number of terms
     d dirs_c                                d in_c + sum_k 2^k (d in_sin cos - d in_cos sin): the terms' bounds + (2 Lv + 2) sum |term|
     d W_ji = sum_r d_rj x_ri, d b_j         per term E_d |x| + |d| E_x + |term|;  the sum: a workgroup adds its rays in order, the
                                             workgroups' sums are added in order -> (rays per workgroup + workgroups) sum |term|
   tree(R) restates the library's split of R rays over workgroups (csrc/evd_voxel_color_api.hip cr_rays_per_block).
"""
import numpy as np
import torch

from composite_ref import _act, _code, _f64, _scan, form
from torch_restatement import embed

FEAT_FAULTS = ("no_act_grad", "T_i", "suffix_incl", "drop_last_geo")
COLOR_FAULTS = ("transposed_w1", "drop_last_geo", "sincos_swapped")


# ---- 1. the feature composite ------------------------------------------------------------------------------------------------------
def feat_composite_bwd(sigma, rows, z, rays_d, g_fmap=None, g_depth=None, g_acc=None, g_w=None, rows_act="relu", sigma_act="relu",
                       rmnear=0.0, noise=None, fault=None):
    """sigma [R, S] (the density channel of raw), rows [R, S, G] before the activation, z [R, S], rays_d [R, >= 3], noise [R, S - 1];
    upstream gradients, None = zero.  -> d_sigma [R, S] (last column 0), d_rows [R, S, G], d_rays_d [R, 3] and E_<name>"""
    dev = rows.device if isinstance(rows, torch.Tensor) else "cpu"
    rows, sigma = _f64(rows, dev), _f64(sigma, dev)
    R, S, G = rows.shape
    fm = form("bwd", S)
    q = _scan(torch.cat([sigma[..., None], rows], -1), z, rays_d, 0, 1, G, rows_act, sigma_act, rmnear, noise, fm, 0.0)
    zero = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    gm = _f64(g_fmap, dev) if g_fmap is not None else zero(R, G)
    gd = _f64(g_depth, dev) if g_depth is not None else zero(R)
    ga = _f64(g_acc, dev) if g_acc is not None else zero(R)
    gw = _f64(g_w, dev) if g_w is not None else zero(R, S)
    a, E_a, da, E_da = q["rgb"], q["E_rgb"], q["drgb"], q["E_drgb"]
    zz, w, T1 = q["z"], q["w"], q["T_next"]
    gm_dot = gm.clone()
    if fault == "drop_last_geo":
        gm_dot[:, -1] = 0
    t = gm_dot[:, None, :] * a
    dot, M_dot = t.sum(-1), t.abs().sum(-1)
    E_dot = (gm.abs()[:, None, :] * E_a).sum(-1) + (G + 1) * M_dot
    Gi = dot + gd[:, None] * zz + ga[:, None] + gw
    MG = M_dot + (gd[:, None] * zz).abs() + ga.abs()[:, None] + gw.abs()
    E_G = E_dot + 5 * MG
    Gw = Gi * w
    E_Gw = E_G * w.abs() + Gi.abs() * q["E_w"] + Gw.abs()
    suffix = Gw.flip(1).cumsum(1).flip(1) - (0 if fault == "suffix_incl" else Gw)
    E_suffix = E_Gw.sum(1, keepdim=True) + (fm["n_sum"] + 1) * Gw.abs().sum(1, keepdim=True)
    Tq = q["T"] if fault == "T_i" else T1
    qd = q["dist"] * (Gi[:, :-1] * Tq[:, :-1] - suffix[:, :-1])
    E_q = q["dist"].abs() * (E_G[:, :-1] * T1[:, :-1].abs() + Gi[:, :-1].abs() * q["E_Tn"][:, :-1] + E_suffix
                             + 2 * ((Gi * T1)[:, :-1].abs() + Gw.abs().sum(1, keepdim=True))) + 6 * qd.abs()
    d_sigma, E_ds = zero(R, S), zero(R, S)
    d_sigma[:, :-1] = qd * q["mask"] * q["dact"]
    E_ds[:, :-1] = q["mask"] * (q["dact"].abs() * E_q + qd.abs() * q["E_dact"])
    dav = torch.ones_like(da) if fault == "no_act_grad" else da
    d_rows = gm_dot[:, None, :] * w[..., None] * dav
    E_d_rows = gm.abs()[:, None, :] * (q["E_w"][..., None] * da.abs() + w.abs()[..., None] * E_da + 2 * (w[..., None] * da).abs())
    dens = q["dens"]
    dn = (qd * dens).sum(1)
    E_dn = (E_q * dens.abs() + qd.abs() * q["E_dens"] + (qd * dens).abs()).sum(1) + (fm["n_sum"] + 1) * (qd * dens).abs().sum(1)
    n2 = q["norm"][:, 0] ** 2
    return dict(d_sigma=d_sigma, E_d_sigma=E_ds, d_rows=d_rows, E_d_rows=E_d_rows, d_rays_d=(dn / n2)[:, None] * q["d"],
                E_d_rays_d=(q["d"].abs() / n2[:, None]) * (E_dn + 8 * dn.abs())[:, None], act_rows=a, weights=w)


def feat_composite_autograd(sigma, rows, z, rays_d, rows_act="relu", sigma_act="relu", rmnear=0.0, noise=None):
    """the forward as plain torch ops (voxnerf.py:153-201,223-229) for float64 autograd: (fmap [R, G], acc, weights, depth)"""
    z = torch.as_tensor(z).double()
    dists = (z[:, 1:] - z[:, :-1]) * rays_d[:, None, :3].norm(dim=-1)
    a = _act(_code(rows_act), rows, torch.zeros_like(rows))[0]
    y = sigma[:, :-1] + (torch.as_tensor(noise).double() if noise is not None else 0.0)
    dens = _act(_code(sigma_act), y, torch.zeros_like(y))[0]
    if rmnear > 0:
        dens = (z[:, 1:].float() > float(np.float32(rmnear))).double() * dens
    alpha = torch.cat([1 - torch.exp(-dens * dists), torch.ones_like(z[:, :1])], -1)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(z[:, :1]), 1 - alpha], -1), -1)[:, :-1]
    return (w[..., None] * a).sum(-2), w.sum(-1), w, (w * z).sum(-1)


# ---- 2. the per-ray colour network -------------------------------------------------------------------------------------------------
MAX_BLOCKS = 256


def tree(R):
    """(rays per workgroup, workgroups) of the colour network's backward for R rays"""
    rpb = 4 * -(-(-(-R // 4)) // MAX_BLOCKS)
    return rpb, -(-R // rpb)


def color_params(sd, dev="cpu"):
    """{w0, b0, w1, b1, w2, b2} float64 from a level's state dict (absent biases: None)"""
    P = {}
    for l in range(3):
        P[f"w{l}"] = _f64(np.asarray(sd[f"color_net.{l}.weight"]), dev)
        k = f"color_net.{l}.bias"
        P[f"b{l}"] = _f64(np.asarray(sd[k]), dev) if k in sd else None
    return P


def _lin(W, b, x, E_x):
    y = x @ W.T
    M = x.abs() @ W.abs().T
    if b is not None:
        y, M = y + b, M + b.abs()
    return y, E_x @ W.abs().T + (W.shape[1] + 1) * M


def _lin_t(W, d, E_d):
    """W^T d: rows of d [R, out] -> [R, in]"""
    return d @ W, E_d @ W.abs() + (W.shape[0] + 1) * (d.abs() @ W.abs())


def color_rows(P, fmap, dirs, Lv, g_color=None, fault=None):
    """P from color_params; fmap [R, G], dirs [R, >= 3] (float32 values), g_color [R, 3] or None (forward only).
    -> color, E_color, unsure [R] and, with g_color: d_map, d_dirs, d_w0 .. d_b2 with E_<name>"""
    dev = fmap.device if isinstance(fmap, torch.Tensor) else "cpu"
    fmap, dirs = _f64(fmap, dev), _f64(dirs, dev)[:, :3]
    R, G = fmap.shape
    w0, w1, w2 = P["w0"], P["w1"], P["w2"]
    if fault == "transposed_w1":
        w1 = w1.T
    enc = embed(dirs, Lv)
    if fault == "sincos_swapped":
        enc = torch.cat([dirs] + [f(dirs * 2.0 ** k) for k in range(Lv) for f in (torch.cos, torch.sin)], -1)
    E_enc = torch.cat([torch.zeros_like(dirs), 4 * enc[:, 3:].abs()], -1)
    fin = fmap.clone()
    if fault == "drop_last_geo":
        fin[:, -1] = 0
    x, E_x = torch.cat([fin, enc], -1), torch.cat([torch.zeros_like(fmap), E_enc], -1)
    y0, E_y0 = _lin(w0, P["b0"], x, E_x)
    m0 = (y0 > 0).double()
    h0, E_h0 = y0 * m0, E_y0 * m0
    y1, E_y1 = _lin(w1, P["b1"], h0, E_h0)
    m1 = (y1 > 0).double()
    h1, E_h1 = y1 * m1, E_y1 * m1
    y2, E_y2 = _lin(w2, P["b2"], h1, E_h1)
    s, E_s, ds, _ = _act(2, y2, E_y2)
    U = 2.0 ** -24
    unsure = ((y0.abs() <= 4 * U * E_y0) & (E_y0 > 0)).any(-1) | ((y1.abs() <= 4 * U * E_y1) & (E_y1 > 0)).any(-1)
    out = dict(color=s, E_color=E_s, unsure=unsure, h0=h0, h1=h1)
    if g_color is None:
        return out
    g = _f64(g_color, dev)
    d2 = g * ds
    E_d2 = g.abs() * ((1 - 2 * s).abs() * E_s + 4 * ds)
    dh1, E_dh1 = _lin_t(w2, d2, E_d2)
    dh1, E_dh1 = dh1 * m1, E_dh1 * m1
    dh0, E_dh0 = _lin_t(w1, dh1, E_dh1)
    dh0, E_dh0 = dh0 * m0, E_dh0 * m0
    dx, E_dx = _lin_t(w0, dh0, E_dh0)
    d_map = dx[:, :G].clone()
    if fault == "drop_last_geo":
        d_map[:, -1] = 0
    d_dirs, E_dd, M_dd = dx[:, G:G + 3].clone(), E_dx[:, G:G + 3].clone(), dx[:, G:G + 3].abs()
    for k in range(Lv):
        f = 2.0 ** k
        sn, cs = torch.sin(dirs * f), torch.cos(dirs * f)
        gs, gc = dx[:, G + 3 + 6 * k:G + 6 + 6 * k], dx[:, G + 6 + 6 * k:G + 9 + 6 * k]
        Es, Ec = E_dx[:, G + 3 + 6 * k:G + 6 + 6 * k], E_dx[:, G + 6 + 6 * k:G + 9 + 6 * k]
        if fault == "sincos_swapped":
            gs, gc = gc, gs
        t1, t2 = gs * cs * f, -gc * sn * f
        d_dirs = d_dirs + t1 + t2
        E_dd = E_dd + f * (Es * cs.abs() + Ec * sn.abs() + gs.abs() * 4 * cs.abs() + gc.abs() * 4 * sn.abs()) + 2 * (t1.abs() + t2.abs())
        M_dd = M_dd + t1.abs() + t2.abs()
    E_dd = E_dd + (2 * Lv + 2) * M_dd
    out.update(d_map=d_map, E_d_map=E_dx[:, :G], d_dirs=d_dirs, E_d_dirs=E_dd)
    rpb, nb = tree(R)
    n_tree = rpb + nb

    def wsum(d, E_d, xx, E_xx):
        t_abs = d.abs().T @ xx.abs()
        return d.T @ xx, E_d.T @ xx.abs() + d.abs().T @ E_xx + (1 + n_tree) * t_abs

    out["d_w2"], out["E_d_w2"] = wsum(d2, E_d2, h1, E_h1)
    out["d_w1"], out["E_d_w1"] = wsum(dh1, E_dh1, h0, E_h0)
    if fault == "transposed_w1":
        out["d_w1"] = out["d_w1"].T
    out["d_w0"], out["E_d_w0"] = wsum(dh0, E_dh0, x, E_x)
    for l, (d, E_d) in enumerate(((dh0, E_dh0), (dh1, E_dh1), (d2, E_d2))):
        out[f"d_b{l}"], out[f"E_d_b{l}"] = d.sum(0), E_d.sum(0) + n_tree * d.abs().sum(0)
    return out


def color_rows_autograd(P, fmap, dirs, Lv):
    """plain torch ops (voxnerf.py:231-239) for float64 autograd"""
    h = torch.cat([fmap, embed(dirs[:, :3], Lv)], -1)
    for l in range(3):
        h = h @ P[f"w{l}"].T
        if P[f"b{l}"] is not None:
            h = h + P[f"b{l}"]
        h = torch.relu(h) if l < 2 else torch.sigmoid(h)
    return h


# ---- the cases of tests/test_gpu_pbe_kernels.py, built on the CPU (seeds chosen there, see tests/test_pbe_level_ref.py) ---------------
def feat_case(R, S, G, sub="all", noise=False, act="relu", stride=3, seed=0):
    return dict(id=f"{R}x{S}x{G}-g_{sub}-{'noise' if noise else 'nonoise'}-{act}-stride{stride}", R=R, S=S, G=G, sub=sub, noise=noise, act=act,
                stride=stride, seed=seed)


FEAT_SHAPES = [(1, 1, 15), (1, 2, 1), (5, 63, 15), (4, 64, 15), (3, 65, 15), (5, 128, 16), (2, 129, 17), (2, 256, 128), (257, 64, 15)]


def _feat_cases():
    out = [feat_case(R, S, G, seed=1000 + i) for i, (R, S, G) in enumerate(FEAT_SHAPES)]
    k = 0
    for (R, S, G) in ((5, 63, 15), (3, 65, 15), (5, 128, 16), (257, 64, 15)):
        for sub in ("fmap", "all", "w"):
            for noise in (False, True):
                k += 1
                out.append(feat_case(R, S, G, sub, noise, ("relu", "none")[k % 2], (3, 11)[(k // 2) % 2], seed=2000 + k))
    seen, uniq = set(), []
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


FEAT_CASES = _feat_cases()


_CACHE = {}


def _cached(fn):
    def f(c, *a):
        key = (fn.__name__, c["id"]) + a
        if key not in _CACHE:
            _CACHE[key] = fn(c, *a)
        return _CACHE[key]
    f.__doc__ = fn.__doc__
    return f


@_cached
def feat_inputs(c):
    """float32 numpy inputs, shared (do not write): raw [R, S, 4] (sigma in channel 0, the others junk the kernel must not read), rows, z,
    rays [R, stride] (the direction in columns 3..5 of an 11-column ray batch, else 0..2), noise | None, g = (g_fmap, g_depth, g_acc, g_w)
    with None for the missing ones.  Rows 1, 2, 3 (where they exist) hold an opaque sample, all non-positive densities, duplicate z."""
    R, S, G = c["R"], c["S"], c["G"]
    for seed in range(c["seed"], c["seed"] + 100):          # the first seed whose geo pre-activations are >= 25 % positive and >= 25 % not
        rs = np.random.RandomState(seed)
        raw = rs.normal(size=(R, S, 4)).astype(np.float32)
        raw[..., 0] *= rs.choice([0.5, 5.0, 50.0], size=(R, 1)).astype(np.float32)
        rows = rs.normal(size=(R, S, G)).astype(np.float32)
        if 0.25 <= float((rows > 0).mean()) <= 0.75:
            break
    raw[0, 0, 0] = abs(raw[0, 0, 0]) + 0.5                   # (the one-ray cases: a density sample that carries weight)
    z = np.sort(2 + 4 * rs.uniform(size=(R, S)), -1).astype(np.float32)
    if R > 1 and S > 2:
        raw[1, S // 3, 0] = 1e6
    if R > 2:
        raw[2, :, 0] = -np.abs(raw[2, :, 0])
    if R > 3 and S > 2:
        z[3, S // 2] = z[3, S // 2 - 1]
    rays = rs.normal(size=(R, c["stride"])).astype(np.float32)
    noise = rs.normal(size=(R, S - 1)).astype(np.float32) if (c["noise"] and S > 1) else None
    gs = [rs.normal(size=sh).astype(np.float32) for sh in ((R, G), (R,), (R,), (R, S))]
    keep = {"all": (0, 1, 2, 3), "fmap": (0,), "w": (3,)}[c["sub"]]
    return dict(raw=raw, rows=rows, z=z, rays=rays, col=3 if c["stride"] == 11 else 0, noise=noise,
                g=tuple(gs[i] if i in keep else None for i in range(4)))


def feat_reference(c, dev="cpu", fault=None):
    a = feat_inputs(c)
    t = lambda v: None if v is None else torch.as_tensor(v).to(dev)
    rd = t(a["rays"])[:, a["col"]:a["col"] + 3]
    return feat_composite_bwd(t(a["raw"])[..., 0], t(a["rows"]), t(a["z"]), rd, *[t(v) for v in a["g"]], rows_act=c["act"],
                              noise=t(a["noise"]), fault=fault)


COLOR_R = (1, 4, 5, 257)
COLOR_LV = (0, 3, 4)
UNSURE_CAP = 0.02
# (R, Lv, bias) -> the first seed from 0 whose `unsure` rays stay within UNSURE_CAP of the case's rays (tests/test_pbe_level_ref.py
# asserts that these are the ones choose_color_seed finds)
COLOR_SEEDS = {(R, Lv, b): 0 for R in COLOR_R for Lv in COLOR_LV for b in (True, False)}
COLOR_SEEDS.update({(4, 3, False): 1, (257, 4, True): 2})


def color_case(R, Lv, bias, accumulate, want_dirs, stride):
    return dict(id=f"R{R}-Lv{Lv}-{'bias' if bias else 'nobias'}-acc{int(accumulate)}-{'dirs' if want_dirs else 'nodirs'}-stride{stride}", R=R, Lv=Lv,
                bias=bias, accumulate=accumulate, want_dirs=want_dirs, stride=stride)


def _color_cases():
    out, k = [], 0
    for R in COLOR_R:
        for Lv in COLOR_LV:
            k += 1
            out.append(color_case(R, Lv, bool(k % 2), bool((k // 2) % 2), bool((k // 3) % 2), (3, 11)[k % 2]))
            out.append(color_case(R, Lv, not k % 2, not (k // 2) % 2, not (k // 3) % 2, (3, 11)[(k + 1) % 2]))
    return out


COLOR_CASES = _color_cases()


def color_state_dict(c):
    """the coarse level's weights with the case's direction encoding and bias choice (voxel_level_ref's seeds and shapes)"""
    import voxel_level_ref as V
    return V._state_dict("coarse", (10, c["Lv"]), c["bias"])


def _color_draw(c, seed):
    rs = np.random.RandomState(7000 + seed)
    R = c["R"]
    fmap = np.abs(rs.normal(size=(R, 15))).astype(np.float32)
    d = rs.normal(size=(R, 3))
    rays = rs.normal(size=(R, c["stride"])).astype(np.float32)
    col = 3 if c["stride"] == 11 else 0
    rays[:, col:col + 3] = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    return dict(fmap=fmap, rays=rays, col=col, g_color=rs.normal(size=(R, 3)).astype(np.float32))


def _color_unsure(c, a):
    P = color_params(color_state_dict(c))
    return color_rows(P, torch.as_tensor(a["fmap"]), torch.as_tensor(a["rays"])[:, a["col"]:a["col"] + 3], c["Lv"])["unsure"].numpy()


@_cached
def color_inputs(c, seed=None):
    """float32 numpy: fmap [R, 15] (composited relu rows: non-negative), rays [R, stride] with unit directions, g_color [R, 3], unsure [R].
    The rays a ReLU may decide differently on in float32 (`unsure`, from the float64 forward alone) are left out of the comparison: their
    colour and d_map rows are not compared, and their g_color rows are zero, which takes their terms out of the weight-gradient sums of
    the kernel and of the reference alike."""
    seed = COLOR_SEEDS[(c["R"], c["Lv"], c["bias"])] if seed is None else seed
    a = _color_draw(c, seed)
    a["unsure"] = _color_unsure(c, a)
    a["g_color"][a["unsure"]] = 0
    return a


def color_reference(c, dev="cpu", fault=None, seed=None):
    a = color_inputs(c, seed)
    t = lambda v: torch.as_tensor(v).to(dev)
    return color_rows(color_params(color_state_dict(c), dev), t(a["fmap"]), t(a["rays"])[:, a["col"]:a["col"] + 3], c["Lv"], t(a["g_color"]), fault=fault)


def choose_color_seed(c, limit=64):
    for seed in range(limit):
        if _color_unsure(c, _color_draw(c, seed)).sum() <= UNSURE_CAP * c["R"]:
            return seed
    raise RuntimeError(f"no seed below {limit} keeps the unsure rays of {c['id']} within {UNSURE_CAP:g}")
