"""float64 reference of the compositing scan (raw2outputs, nerf.py:74-129 / voxnerf.py:153-201), of its backward, and of the
importance resampling (sample_pdf + merge + z_std, utils/rays.py:149-193, renderer.py:200-250), with a first-order error bound for
every output.  Test infrastructure only.

Kept in float32 on purpose, because the kernels and the reference must agree on them bit for bit:
  - z_mid = 0.5 * (z[i] + z[i + 1]), one float32 add and an exact halving (renderer.py:200 on float32 tensors);
  - the cdf knots: float32 of the float64 prefix of float32(float32(w + 1e-5) / float32(exact sum)), as k_sample_pdf_merge documents.
    For weights in [0, 1] and S <= 257 the float64 prefix is exact (dynamic range < 2^29), so any scan order gives these bits;
  - the searchsorted(right=True) index taken on those knots, and the `denom < 1e-5` guard decided on the float32 knot difference.
  - the constants of sigmoid1 (1.002, 0.001) and the rmnear threshold are the float32 numbers a float32 torch graph multiplies by.
Everything after the knots, and every step of the scan, is float64.

The reference's `- alpha + (1. + 1e-10)` (nerf.py:116, voxnerf.py:186) is left out: no kernel has it, and it is not a no-op.  Behind a
sample whose alpha is 1 to float32 precision the reference's transmittance is ~1e-10 instead of ~0, so each of its S weights is off by
at most 1e-10 (`eps` below restores the term; tests/test_composite_ref.py pins both forms to the goldens and bounds the difference).

Error model.  A kernel form is described by the number of roundings along any path of its row sums (`n_sum`: chunks or samples per
lane plus the DPP tree) and whether it evaluates exp with the hardware exp2 (`fast_exp`: the argument is scaled by log2(e) first, one
more rounding of |x|).  Every bound below is in units of u = 2^-24, first order, with the form's counts:
  dist = (z1 - z0) |d|           dz 1, the float32 norm 2.5, the product 1                               -> 5 |dist|
  density = act(raw [+ noise])   the activation's own error (per code, see _act) and the noise add's rounding through act'
  x = density dist, e = exp(-x)  E_x = |dist| E_dens + |dens| E_dist + (1 + fast_exp) |x|;  E_e = e (E_x + 2)
  alpha = 1 - e, om = 1 - alpha  E_alpha = E_e + |alpha|,  E_om = E_alpha + |om|  (at alpha -> 1, om is ~u absolute, not relative)
  T_i = prod_{j<i} om_j          E_T(i+1) = E_T(i) |om_i| + |T_i| E_om(i) + |T_(i+1)|  + 3 |T_i| (the chunk carries): one rounding per
                                 factor whatever the association, and an opaque sample's om error enters absolutely
  w = alpha T                    E_w = |T| E_alpha + |alpha| E_T + |w|
  acc, depth, rgb, features      sum of the terms' bounds + (n_sum + 1) sum |term|; white background + E_acc + |1 - acc| + |rgb|
The backward (hand-written, the kernel's decomposition G_i = dL/dw_i, dL/d density_i = dist_i (G_i T_(i+1) - sum_{j>i} G_j w_j)):
  G_i                            sum |g_map_c| E_rgb + 6 (|g_map . rgb| + |g_depth z| + |g_acc| + sum |g_map| + |g_w|)
  suffix (total - prefix)        sum over the WHOLE row of E(G_j w_j) + (n_sum + 1) sum_j |G_j w_j|: the kernel subtracts two prefix sums
  dL/d density, d raw            |dist| (E_G |T_(i+1)| + |G| E_T + E_suffix + 2 (|G T| + sum |G w|)) + 6 |q|;  x |act'| + |q| E_act'
  d rays_d                       |d_c| / |d|^2 (E_dn + 8 |dn|),  dn = sum_i q_i density_i
  act' of sigmoid / sigmoid1      s (1 - s) with s rounded: the 1 - s cancels, so its bound has an absolute part 4 s^2 (the saturated
                                 derivative is ~u, not relatively accurate -- as in torch's float32 sigmoid backward)
  white background               d (1 - acc) / d raw = 0 exactly: the last alpha is 1, so acc = 1 and sum_{j>i} w_j = T_(i+1); the
                                 kernel's `- sum g_map` in G changes only rounding
"""
import numpy as np
import torch

ACT = {"none": 0, "relu": 1, "sigmoid": 2, "exp": 3, "sigmoid1": 4, "softplus": 5, "tanh": 6}
S1_A, S1_B = float(np.float32(1.002)), float(np.float32(0.001))

# kernel forms: n_sum = roundings along any path of a row sum; fast_exp = __expf (hardware exp2 of x log2 e)
def form(name, S):
    nch, spl = -(-S // 64), -(-S // 64)
    if name == "il":
        return dict(n_sum=nch - 1 + 6, fast_exp=True)
    if name in ("rows", "bwd"):
        return dict(n_sum=spl - 1 + 7, fast_exp=False)
    if name == "composite":
        return dict(n_sum=nch - 1 + 6, fast_exp=False)
    if name == "weighted":                  # k_composite<0> for the scan, k_weighted_channels (sequential over S) for the maps
        return dict(n_sum=nch - 1 + 6, fast_exp=False, map_sum=S)
    raise KeyError(name)


def _code(a):
    return ACT[a] if isinstance(a, str) else int(a)


def _act(code, y, e_y):
    """float64 activation (torch semantics: relu propagates NaN), its error bound E (units of u) given the input's bound e_y, its
    derivative and the derivative's bound"""
    if code == 1:
        v = torch.relu(y)
        pos = (y > 0).double()
        return v, e_y * pos, pos, torch.zeros_like(y)
    if code == 2:
        s = torch.sigmoid(y)
        d = s * (1 - s)
        return s, s * (5 + y.abs() * (1 - s)) + e_y * d, d, d * (6 + y.abs()) + 4 * s * s      # act_grad's 1 - s cancels: ~u absolute
    if code == 3:
        v = torch.exp(y)
        return v, v * (2 + e_y), v, v * (2 + e_y + 1)
    if code == 4:
        s = torch.sigmoid(y)
        v = S1_A * s - S1_B
        d = S1_A * s * (1 - s)
        return v, v.abs() + S1_A * s * (5 + y.abs() * (1 - s)) + e_y * d, d, d * (7 + y.abs()) + 5 * s * s
    if code == 5:
        t = y - 1
        big = t > 20
        v = torch.where(big, t, torch.nn.functional.softplus(torch.where(big, torch.zeros_like(t), t), beta=1, threshold=1e30))
        d = torch.where(big, torch.ones_like(t), torch.sigmoid(t))
        e_t = e_y + t.abs()                  # the float32 x - 1
        E = torch.where(big, e_t, 2 * v.abs() + d * (2 + e_t))
        return v, E, d, torch.where(big, torch.zeros_like(t), d * (6 + t.abs()))
    if code == 6:
        v = torch.tanh(y)
        d = 1 - v * v
        return v, 4 * v.abs() + e_y * d, d, 8 * v * v + d * (1 + e_y)
    return y, e_y, torch.ones_like(y), torch.zeros_like(y)


def _f64(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.float64)


def _scan(raw, z, rays_d, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, rmnear, noise, fm, eps):
    """the forward quantities every output is built from, with their bounds"""
    dev = raw.device
    R, S, _ = raw.shape
    z = _f64(z, dev)
    d = _f64(rays_d, dev)[:, :3]
    norm = d.norm(dim=-1, keepdim=True)
    dist = (z[:, 1:] - z[:, :-1]) * norm
    E_dist = 5 * dist.abs()
    y = raw[:, :-1, sigma_ch]
    e_y = torch.zeros_like(y)
    if noise is not None:
        y = y + _f64(noise, dev)
        e_y = y.abs()
    dens, E_dens, dact, E_dact = _act(_code(sigma_act), y, e_y)
    mask = torch.ones_like(dens)
    if rmnear > 0:
        z32 = torch.as_tensor(z[:, 1:]).float()
        mask = (z32 > float(np.float32(rmnear))).double()
        dens, E_dens = mask * dens, mask * E_dens
    x = dens * dist
    E_x = dist.abs() * E_dens + dens.abs() * E_dist + (2 if fm["fast_exp"] else 1) * x.abs()
    e = torch.exp(-x)
    E_e = e * (E_x + 2)
    one = torch.ones_like(z[:, :1])
    zero = torch.zeros_like(z[:, :1])
    alpha = torch.cat([1 - e, one], 1)
    E_alpha = torch.cat([E_e + (1 - e).abs(), zero], 1)
    om = torch.cat([e, zero], 1) + eps                        # eps = 1e-10: the reference's stabiliser (left out by default)
    E_om = E_alpha + om.abs()
    T = torch.cumprod(torch.cat([one, om[:, :-1]], 1), 1)
    E_T = torch.empty_like(T)
    acc_e = torch.zeros_like(z[:, 0])
    for i in range(S):                                        # the running bound of the product scan
        E_T[:, i] = acc_e + 3 * T[:, i].abs()
        acc_e = acc_e * om[:, i].abs() + T[:, i].abs() * E_om[:, i] + (T[:, i] * om[:, i]).abs()
    T_next = torch.cat([T[:, 1:], (T[:, -1] * om[:, -1])[:, None]], 1)
    E_Tn = torch.cat([E_T[:, 1:], acc_e[:, None]], 1)
    w = alpha * T
    E_w = T.abs() * E_alpha + alpha.abs() * E_T + w.abs()
    yc = raw[:, :, rgb_ch0:rgb_ch0 + n_rgb]
    rgb, E_rgb, drgb, E_drgb = _act(_code(rgb_act), yc, torch.zeros_like(yc))
    return dict(z=z, d=d, norm=norm, dist=dist, E_dist=E_dist, dens=dens, E_dens=E_dens, dact=dact, E_dact=E_dact, mask=mask,
                alpha=alpha, T=T, E_T=E_T, T_next=T_next, E_Tn=E_Tn, w=w, E_w=E_w, rgb=rgb, E_rgb=E_rgb, drgb=drgb, E_drgb=E_drgb)


def _wsum(w, E_w, v, E_v, n):
    """sum_i w_i v_i over the last sample axis (v [R, S, K]) and its bound"""
    t = w[..., None] * v
    return t.sum(1), (E_w[..., None] * v.abs() + w.abs()[..., None] * E_v + t.abs()).sum(1) + n * t.abs().sum(1)


def composite(raw, z, rays_d, sigma_ch=3, rgb_ch0=0, n_rgb=3, rgb_act="sigmoid", sigma_act="relu", white=False, rmnear=0.0,
              noise=None, feature=None, form_name="composite", eps=0.0):
    """raw [R, S, C] (torch, any device), z [R, S], rays_d [R, >= 3] (rows of any stride: columns 0..2 are the direction), noise
    [R, S - 1], feature [R, S, F].  Returns rgb (the map of n_rgb channels), density, acc, weights, depth, fmap and E_<name> (the bound
    of each, in units of u, for the kernel form `form_name`)."""
    dev = raw.device if isinstance(raw, torch.Tensor) else "cpu"
    raw = _f64(raw, dev)
    R, S, _ = raw.shape
    fm = form(form_name, S)
    q = _scan(raw, z, rays_d, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, rmnear, noise, fm, eps)
    w, E_w, zz = q["w"], q["E_w"], q["z"]
    n = fm["n_sum"] + 1
    nm = fm.get("map_sum", fm["n_sum"]) + 1
    acc, E_acc = _wsum(w, E_w, torch.ones_like(w)[..., None], torch.zeros_like(w)[..., None], n)
    depth, E_depth = _wsum(w, E_w, zz[..., None], torch.zeros_like(w)[..., None], n)
    rgb, E_rgb = _wsum(w, E_w, q["rgb"], q["E_rgb"], nm)
    if white:
        acc_m, E_acc_m = _wsum(w, E_w, torch.ones_like(w)[..., None], torch.zeros_like(w)[..., None], nm)
        rgb = rgb + (1 - acc_m)
        E_rgb = E_rgb + E_acc_m + (1 - acc_m).abs() + rgb.abs()
    out = dict(rgb=rgb, E_rgb=E_rgb, acc=acc[:, 0], E_acc=E_acc[:, 0], depth=depth[:, 0], E_depth=E_depth[:, 0], weights=w,
               E_weights=E_w, density=q["dens"], E_density=q["E_dens"], scan=q)
    if feature is not None:
        f = _f64(feature, dev)
        out["fmap"], out["E_fmap"] = _wsum(w, E_w, f, torch.zeros_like(f), S)
    return out


def composite_bwd(raw, z, rays_d, g_map=None, g_depth=None, g_acc=None, g_w=None, sigma_ch=3, rgb_ch0=0, rgb_act="sigmoid",
                  sigma_act="relu", white=False, rmnear=0.0, noise=None, form_name="bwd"):
    """hand-written float64 backward (C = 4, three colours): d raw [R, S, 4] and d rays_d [R, 3] from any subset of the upstream
    gradients (None = zero), with the bounds E_d_raw, E_d_rays_d (units of u)"""
    dev = raw.device if isinstance(raw, torch.Tensor) else "cpu"
    raw = _f64(raw, dev)
    R, S, C = raw.shape
    fm = form(form_name, S)
    q = _scan(raw, z, rays_d, sigma_ch, rgb_ch0, 3, rgb_act, sigma_act, rmnear, noise, fm, 0.0)
    zero = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)
    gm = _f64(g_map, dev) if g_map is not None else zero(R, 3)
    gd = _f64(g_depth, dev) if g_depth is not None else zero(R)
    ga = _f64(g_acc, dev) if g_acc is not None else zero(R)
    gw = _f64(g_w, dev) if g_w is not None else zero(R, S)
    ga_m = ga.abs()
    if white:
        ga = ga - gm.sum(1)
        ga_m = ga_m + gm.abs().sum(1)
    rgb, zz, w, T1 = q["rgb"], q["z"], q["w"], q["T_next"]
    G = (gm[:, None, :] * rgb).sum(-1) + gd[:, None] * zz + ga[:, None] + gw
    MG = (gm[:, None, :] * rgb).abs().sum(-1) + (gd[:, None] * zz).abs() + ga_m[:, None] + gw.abs()
    E_G = (gm.abs()[:, None, :] * q["E_rgb"]).sum(-1) + 6 * MG
    Gw = G * w
    E_Gw = E_G * w.abs() + G.abs() * q["E_w"] + Gw.abs()
    suffix = Gw.flip(1).cumsum(1).flip(1) - Gw                 # sum_{j > i}
    E_suffix = E_Gw.sum(1, keepdim=True) + (fm["n_sum"] + 1) * Gw.abs().sum(1, keepdim=True)
    qd = q["dist"] * (G[:, :-1] * T1[:, :-1] - suffix[:, :-1])             # dL / d density_i, i < S - 1
    E_q = q["dist"].abs() * (E_G[:, :-1] * T1[:, :-1].abs() + G[:, :-1].abs() * q["E_Tn"][:, :-1] + E_suffix
                             + 2 * ((G * T1)[:, :-1].abs() + Gw.abs().sum(1, keepdim=True))) + 6 * qd.abs()
    ds = qd * q["mask"] * q["dact"]
    E_ds = q["mask"] * (q["dact"].abs() * E_q + qd.abs() * q["E_dact"])
    d_raw, E_d_raw = zero(R, S, C), zero(R, S, C)
    drgb = gm[:, None, :] * w[..., None] * q["drgb"]
    E_drgb = gm.abs()[:, None, :] * (q["E_w"][..., None] * q["drgb"].abs() + w.abs()[..., None] * q["E_drgb"] + 2 * (w[..., None] * q["drgb"]).abs())
    d_raw[:, :, rgb_ch0:rgb_ch0 + 3], E_d_raw[:, :, rgb_ch0:rgb_ch0 + 3] = drgb, E_drgb
    d_raw[:, :-1, sigma_ch], E_d_raw[:, :-1, sigma_ch] = ds, E_ds
    dens = q["dens"]
    dn = (qd * dens).sum(1)
    E_dn = (E_q * dens.abs() + qd.abs() * q["E_dens"] + (qd * dens).abs()).sum(1) + (fm["n_sum"] + 1) * (qd * dens).abs().sum(1)
    n2 = q["norm"][:, 0] ** 2
    d_rd = (dn / n2)[:, None] * q["d"]
    E_d_rd = (q["d"].abs() / n2[:, None]) * (E_dn + 8 * dn.abs())[:, None]
    return dict(d_raw=d_raw, E_d_raw=E_d_raw, d_rays_d=d_rd, E_d_rays_d=E_d_rd)


def composite_autograd(raw, z, rays_d, sigma_ch=3, rgb_ch0=0, rgb_act="sigmoid", sigma_act="relu", white=False, rmnear=0.0, noise=None,
                       eps=0.0):
    """the same forward written as plain torch ops (nerf.py:74-129), for float64 autograd: (rgb, acc, weights, depth)"""
    z = torch.as_tensor(z).double()
    dists = (z[:, 1:] - z[:, :-1]) * rays_d[:, None, :3].norm(dim=-1)
    rgb = _act(_code(rgb_act), raw[..., rgb_ch0:rgb_ch0 + 3], torch.zeros_like(raw[..., :3]))[0]
    y = raw[:, :-1, sigma_ch] + (torch.as_tensor(noise).double() if noise is not None else 0.0)
    dens = _act(_code(sigma_act), y, torch.zeros_like(y))[0]
    if rmnear > 0:
        dens = (z[:, 1:].float() > float(np.float32(rmnear))).double() * dens
    alpha = torch.cat([1 - torch.exp(-dens * dists), torch.ones_like(z[:, :1])], -1)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(z[:, :1]), 1 - alpha + eps], -1), -1)[:, :-1]
    acc = w.sum(-1)
    rgb_map = (w[..., None] * rgb).sum(-2) + ((1 - acc[:, None]) if white else 0)
    return rgb_map, acc, w, (w * z).sum(-1)


# ---- sample_pdf + merge ---------------------------------------------------------------------------------------------------------
def linspace32(N):
    """linspace(0, 1, N) in float32 as linspace_at (evd_common.h) and the oracle compute it: ATen's symmetric fill"""
    if N == 1:
        return np.zeros(1, np.float32)
    step = np.float32(1.0) / np.float32(N - 1)
    i = np.arange(N)
    lo = (np.float32(0.0) + step * i.astype(np.float32)).astype(np.float32)
    hi = (np.float32(1.0) - step * (N - i - 1).astype(np.float32)).astype(np.float32)
    return np.where(i < N // 2, lo, hi).astype(np.float32)


def cdf_knots(w):
    """w [R, nb - 1] float32 (the weights sample_pdf sees) -> the float32 cdf [R, nb] (torch tensors on w's device)"""
    w = torch.as_tensor(w)
    wp = (w.float() + torch.tensor(1e-5, dtype=torch.float32)).float()
    s = wp.double().sum(-1, keepdim=True).float()
    p = (wp / s).float()
    c = p.double().cumsum(-1).float()
    return torch.cat([torch.zeros_like(c[:, :1]), c], -1)


def sample_pdf(bins, w, u):
    """utils/rays.py:149-193 on float32 bins [R, nb], weights [R, nb - 1] and u [R, N] (float32): the float32 knots and index, then
    float64.  Returns samples (float64), their bound E (units of u), and the index (searchsorted, right=True)"""
    bins = torch.as_tensor(bins).float()
    u = torch.as_tensor(u).float().to(bins.device)
    cdf = cdf_knots(torch.as_tensor(w).to(bins.device))
    nb = cdf.shape[-1]
    inds = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True)
    below = (inds - 1).clamp(min=0)
    above = inds.clamp(max=nb - 1)
    c0, c1 = cdf.gather(1, below), cdf.gather(1, above)
    b0, b1 = bins.gather(1, below).double(), bins.gather(1, above).double()
    guard = (c1 - c0) < torch.tensor(1e-5, dtype=torch.float32)                   # float32 difference, float32 1e-5
    denom = torch.where(guard, torch.ones_like(c0, dtype=torch.float64), c1.double() - c0.double())
    t = (u.double() - c0.double()) / denom
    s = b0 + t * (b1 - b0)
    E = s.abs() + 5 * (t * (b1 - b0)).abs()
    return s, E, inds


def z_mid32(z):
    z = torch.as_tensor(z).float()
    return (0.5 * (z[:, 1:] + z[:, :-1])).float()


def sample_pdf_merge(z, w, N, det=True, u=None):
    """renderer.py:200-250 on z [R, S], coarse weights [R, S] (float32): z_samples (float64) + bound, the index, and u used"""
    z = torch.as_tensor(z).float()
    R = z.shape[0]
    if det:
        u = torch.as_tensor(linspace32(N)).to(z.device).expand(R, N)
    s, E, inds = sample_pdf(z_mid32(z), torch.as_tensor(w).float().to(z.device)[:, 1:-1], u)
    return dict(z_samples=s, E_z_samples=E, inds=inds, u=torch.as_tensor(u))


def merge(z, zs):
    """torch.sort(cat(z, z_samples)) with the stable rank (ties: the lower index of the concatenation first): (z_merged, order)"""
    cat = torch.cat([torch.as_tensor(z).float(), torch.as_tensor(zs).float()], -1).cpu().numpy()
    order = np.argsort(cat, -1, kind="stable")
    return np.take_along_axis(cat, order, -1), order.astype(np.int32)


def z_std(zs):
    """torch.std(z_samples, unbiased=False) in float64 of the float32 samples"""
    return torch.as_tensor(zs).double().std(-1, unbiased=False)
