"""float64 reference of the kernels between the AWP embedding and the per-ray tail: the feature_integration scan and its backward
(evd_awp_feature_integration / _bwd: csrc/kernel_awp_integrate.hip + awp_integrate.h), the per-sample part of the MotionAggregationModule
(evd_mam_local_forward / _backward: csrc/kernel_mam.hip) and the fused backward of h_local's two consumers
(evd_awp_local_consumers_backward), with a first-order bound for every forward output, the backward tolerances, the structural FAULTS
the reference can reproduce on request, and the CASES matrix that names the dispatch arm of every case.  Test infrastructure only;
tests/test_awp_local_ref.py pins it on the CPU, tests/test_gpu_awp_local.py holds the kernels to it.

integrate64   awp.py:58-75 AS WRITTEN: zeros appended (the last sample's alpha is 0), cumprod along the CHANNEL axis of the previous
              sample's row, om = 1 - alpha + 1e-10 (evaluated as e + 1e-10, the same number without the cancellation), d feat / d z /
              d rays_d by float64 autograd.
mam_local64   mam.py:72-74, 29-33 reduced to h_local as the header of kernel_mam.hip derives it: logit = u . h, alpha = softmax over s,
              beta = softmax over p, h_inter = sum_s alpha h, h_intra = sum_p beta h;  d h_local and the PER-RAY d u by the kernel
              header's formulas (tests/test_awp_local_ref.py holds them, and the reduction itself, to autograd of the unreduced module).
consumers64   the sum of the two d h_local shares, d z, d rays_d, per-ray d u.

Forward error model.  Units of u = 2^-24, first order, per element, computed in float64 next to the value; the asserted bound is K = 2
times the figure (second-order terms and the association of the DPP scans, as tests/voxel_level_ref.py).  Counts read off the code:
  dist = fl(fl(z1 - z0) |d|)    dz 1, ray_norm 2.5, the product 1                                   5 |dist|   (composite_ref.py)
  x = f dist, e = exp_fast(-x)  the product 1, the scaling by float32(log2 e) 1.25:  E_x = |f| E_dist + 2.25 |x|;  v_exp_f32 is 1 ulp:
                                E_e = e (E_x + 2) + FLUSH  (a result below 2^-126 may be flushed: FLUSH = 2^-126 absolute)
  alpha = fl(1 - e)             E_alpha = E_e + |alpha|
  om = fl(-alpha + 1.f)         awp_fwd_row adds `1.f + 1e-10f`, which IS 1.f: the kernel's om lacks the 1e-10 the float64 value has,
                                E_om = E_alpha + |om| + 1e-10 / u   (absolute; it is the whole of om behind an opaque channel)
  Q[s+1, c] = prod_{c'<=c} om   the recurrence of composite_ref.py's T run along the channels (awp_next_q: lane product, DPP scan and
                                `excl *= om` multiply each factor in once):  E_Q(c) = E_Q(c-1) om^ + Q^(c-1) E_om(c) + Q^(c), with the
                                upper magnitudes om^ = |om| + u E_om, Q^ = prod om^ (loss_ref.py: next to an opaque channel the error of
                                om is as large as om)
  out[c] = sum_s alpha Q f      t = fl(fl(alpha Q) f): |f| (Q^ E_alpha + |alpha| E_Q) + 2 |t|;  S sequential adds: sum E_t + S sum |t|
  logit a = u . h               dot4 (4 products, 3 adds) + row_sum_dpp (4 steps): 8 roundings on sum_c |h_c u_c|
  __expf(a - m)                 m is the maximum of rounded logits: E_m <= max E_a;  the difference 1, the log2 e scaling 1.25:
                                E_x = E_a + max E_a + 2.25 |x|;  E_ex = ex (E_x + 2) + FLUSH
  alpha = ex / t                t: ceil(S / 64) adds per lane + the 6-step tree, E_t = sum E_ex + (ceil(S / 64) + 6) t;  the IEEE
                                division 1:  E_alpha = E_ex / t + alpha E_t / t + alpha
  beta = ex fl(1 / t)           t: P sequential adds;  the reciprocal 1 and the product 1:  E_beta = E_ex / t + beta E_t / t + 2 beta
  h_inter[p] = sum_s alpha h    an FMA chain of ceil(S / 16) steps per lane group, two lane exchanges, the 4-way LDS sum (3 adds):
                                sum_s E_alpha |h| + (ceil(S / 16) + 5) sum_s |alpha h|
  h_intra[s] = sum_p beta h     a P-step FMA chain:  sum_p E_beta |h| + P sum_p |beta h|
  row / column sums             sum_s alpha = 1 within sum_s E_alpha, sum_p beta = 1 within sum_p E_beta (summed in float64 by the test)
Nothing measured on a kernel enters a bound.

Backward tolerances (the project's own figures for these float32 kernels), relative L2 PER RAY -- each ray's slice of d feat / d h_local /
d z / d u -- so that one wrong ray of N is not diluted: scan 1e-5 (test_awp_feature_integration_backward_matches_torch_autograd), MAM
2e-5 (test_mam_local_backward_equals_float64_autograd), the fused sum 2e-5.  d rays_d = dnorm d / |d| is a cancelling sum over the
samples: it is compared per ray against max(|ref|, floor), the floor being where the first-order bound of tests/loss_ref.py
(E_d_rays_d) equals the tolerance, floor = K u E / tol.  Where a ray's float64 gradient is exactly 0 (a zero direction, S = 1) the
kernel's must be exactly 0.

Inputs (make_inputs, reference).  Seeded by the case id: |N(0, 1)| features with per-ray scales from {0.05, 1, 8}, sorted uniform z,
N(0, 1) directions and upstream gradients.  A per-ray relative tolerance only means something where a float32 evaluation of the
as-written formulas is itself well inside it, so three conditions are imposed on the draw and asserted by the CPU test:
  FD_FLOOR <= max f dist <= FD_CAP on every ordinary ray (FD_SAT <= on the saturated ray of a `saturated` case): alpha = fl(1 - e) has
                 u / (f dist) of relative error, so z spans (0, S / 2) and the rays outside the window are scaled to its edge;
  torch float32 of the same formulas within a TENTH of each tolerance on every ray and within every forward bound at factor 1: d z and
                 d u are cancelling sums, about one ray in thirty of these distributions carries 1e-6 ... 6e-6 of float32 noise, and a
                 case that holds such a ray is drawn again (13 of the 90 cases, at most twice);
  the exact zeros: a zero direction and S = 1 give exactly 0 in d feat, d z and d rays_d of that ray in float64.
"""
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24
FLUSH = 2.0 ** -126 / U                 # the flush-to-zero floor in units of u
K = 2.0
LOG2E_REL = 0.25                        # float32(log2 e) is 0.22 u off log2 e
EPS = 1e-10
TOL = {"scan": 1e-5, "mam": 2e-5, "fused": 2e-5}
FD_CAP, FD_SAT, SPREAD = 40.0, 100.0, 60.0      # max f dist of an ordinary ray, min of a saturated one, logit spread of a peaked row
MAM_C, MAM_MAXP, MAM_MAXS = 64, 16, 512
FD_FLOOR = 0.25                         # min of max f dist of an ordinary ray that has an interval at all (see make_inputs)
Z_PER_SAMPLE = 2.0                      # z is drawn from (0, S / 2): a mean interval of ~0.5 whatever S (see make_inputs)
CPL = {"c64": 4, "cpl1": 1, "cpl2": 2, "cpl4": 4, "consumers": 4}


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64).requires_grad_(grad)


# ---- the scan ---------------------------------------------------------------------------------------------------------------------
def scan_arm(C):
    return "c64" if C == 64 else "cpl1" if C <= 64 else "cpl2" if C <= 128 else "cpl4"


def _scan_fwd(f, z, d, fault=None, cpl=1, as_written=False):
    """awp.py:58-75 on tensors of any float type.  as_written: om by the reference's own `-alpha + (1. + 1e-10)` (the float32 evaluation);
    otherwise the same number as e + 1e-10 (no cancellation at alpha -> 1)"""
    C = f.shape[-1]
    norm = torch.norm(d[..., None, :], dim=-1)
    dists = z[..., 1:] - z[..., :-1]
    if fault != "dist_without_norm":
        dists = dists * norm
    e = torch.exp(-f[..., :-1, :] * dists[..., None])
    if fault == "last_alpha_not_zeroed":                                              # the last interval of nerf.py's raw2outputs instead
        e = torch.cat([e, torch.exp(-f[:, -1:, :] * (1e10 * norm)[..., None])], -2)
    else:
        e = torch.cat([e, torch.ones_like(f[:, -1:, :])], -2)                          # zeros appended to alpha
    alpha = -e + 1
    if as_written:
        om = -alpha + (1. + EPS)
    else:
        om = e + (0.0 if fault == "missing_1e-10" else EPS)
    ch = torch.arange(C)
    if fault == "lane_last_channel_dropped" and cpl > 1:
        om = torch.where(ch % cpl == cpl - 1, torch.ones_like(om), om)
    ones = torch.ones_like(f[:, :1])
    if fault == "cumprod_over_samples":
        Q = torch.cumprod(torch.cat([ones, om], -2), -2)[:, :-1]
    elif fault == "q_inclusive_of_own_row":
        Q = torch.cumprod(om, -1)
    else:
        Q = torch.cumprod(torch.cat([ones, om], -2), -1)[:, :-1]
        if fault == "q_exclusive_over_channels":
            Q = torch.cat([torch.ones_like(Q[..., :1]), Q[..., :-1]], -1)
    return torch.sum(alpha * Q * f, dim=-2)


def _scan_bound(f, z, d):
    """E_out [N, C] of the module docstring (float64 tensors, no autograd)"""
    N, S, C = f.shape
    norm = d.norm(dim=-1)
    dist = torch.cat([(z[:, 1:] - z[:, :-1]) * norm[:, None], torch.zeros_like(z[:, :1])], 1)
    E_dist = 5 * dist.abs()
    x = f * dist[..., None]
    E_x = f.abs() * E_dist[..., None] + (2 + LOG2E_REL) * x.abs()
    live = torch.ones((1, S, 1), dtype=torch.float64)
    live[:, -1] = 0
    e = torch.exp(-x)
    E_e = (e * (E_x + 2) + FLUSH) * live
    e = torch.where(live > 0, e, torch.ones_like(e))
    a = (1 - e) * live
    E_a = (E_e + a.abs()) * live
    om = e + EPS
    E_om = E_a + om.abs() + EPS / U
    om_hi = om.abs() + U * E_om
    Qn = torch.cumprod(om, -1)
    Qn_hi = torch.cumprod(om_hi, -1)
    E_Qn = torch.empty_like(Qn)
    run = torch.zeros_like(om[..., 0])
    prev_hi = torch.ones_like(run)
    for c in range(C):
        run = run * om_hi[..., c] + prev_hi * E_om[..., c] + (Qn_hi[..., c] if c > 0 else 0.0)     # the first factor multiplies 1.f: exact
        E_Qn[..., c] = run
        prev_hi = Qn_hi[..., c]
    one = torch.ones_like(f[:, :1])
    Q_hi = torch.cat([one, Qn_hi[:, :-1]], 1)
    Q = torch.cat([one, Qn[:, :-1]], 1)
    E_Q = torch.cat([torch.zeros_like(one), E_Qn[:, :-1]], 1)
    t = a * Q * f
    E_t = f.abs() * (Q_hi * E_a + a.abs() * E_Q) + 2 * t.abs()
    return E_t.sum(1) + S * t.abs().sum(1) + FLUSH


def _unguarded(x, rows, C, Cp):
    """rows of Cp floats read from a flat buffer of `rows` rows of C floats without the `c < C` guard (zeros behind the buffer)"""
    flat = torch.cat([x.reshape(-1), torch.zeros(Cp, dtype=x.dtype)])
    return flat[(torch.arange(rows) * C)[:, None] + torch.arange(Cp)[None, :]]


def _sfx_fault(f, z, d, g, cpl):
    """what d feat gains when the suffix sum over the lanes to the right includes the lane itself (its own channels enter twice)"""
    N, S, C = f.shape
    dist = torch.cat([(z[:, 1:] - z[:, :-1]) * d.norm(dim=-1)[:, None], torch.zeros_like(z[:, :1])], 1)[..., None]
    e = torch.exp(-f * dist)
    e[:, -1] = 1
    om = e + EPS
    Q = torch.cat([torch.ones_like(f[:, :1]), torch.cumprod(om, -1)[:, :-1]], 1)
    G = g[:, None, :] * (1 - e) * f * Q
    Gn = torch.cat([G[:, 1:], torch.zeros_like(G[:, :1])], 1)
    lane = torch.arange(C) // cpl
    extra = Gn @ (lane[:, None] == lane[None, :]).double()
    out = -(extra / om) * dist * e
    out[:, -1] = 0
    return out


def _no_eps_fault(f, z, d):
    """In exact arithmetic the 1e-10 moves nothing visible; it is there for float32, where e underflows to 0 behind f dist > 103 and the
    backward's sfx / om is 0 / 0.  The reference therefore shows this mistake as float32 shows it: NaN wherever float32(e) is 0."""
    dist = torch.cat([(z[:, 1:] - z[:, :-1]) * d.norm(dim=-1)[:, None], torch.zeros_like(z[:, :1])], 1)[..., None]
    e32 = torch.exp(-(f * dist).float())
    bad = (e32 == 0) & (dist > 0)
    return torch.where(bad, torch.full_like(f, float("nan")), torch.zeros_like(f))


def integrate64(feat, z, rays_d, g=None, fault=None):
    """feat [N, S, C], z [N, S], rays_d [N, 3] (the float32 inputs the kernel gets) -> out, E_out (units of u);  with g = d out [N, C]
    also d_feat, d_z, d_rays_d (float64 autograd) and E_d_rays_d (tests/loss_ref.py's first-order bound, for the floor)"""
    f, zz, d = _t64(feat, g is not None), _t64(z, g is not None), _t64(rays_d, g is not None)
    N, S, C = f.shape
    cpl = CPL[scan_arm(C)]
    out = _scan_fwd(f, zz, d, None if fault in SCAN_BWD_FAULTS else fault, cpl)
    r = dict(out=out.detach(), E_out=_scan_bound(f.detach(), zz.detach(), d.detach()))
    if g is None:
        return r
    g64 = _t64(g)
    fp, gp, o = f, g64, out
    if fault == "padding_channels_in_product" and C < 64 * cpl:
        fp = _unguarded(f.detach(), N * S, C, 64 * cpl).reshape(N, S, 64 * cpl).requires_grad_(True)
        gp = _unguarded(g64, N, C, 64 * cpl)
        o = _scan_fwd(fp, zz, d, None, cpl)
    grads = torch.autograd.grad((o * gp).sum(), [fp, zz, d], allow_unused=True) if o.requires_grad else (None, None, None)
    gf, gz, gd = (torch.zeros_like(x) if v is None else v for v, x in zip(grads, (fp, zz, d)))
    gf = gf[..., :C]
    if fault == "suffix_sum_includes_own_lane":
        gf = gf + _sfx_fault(f.detach(), zz.detach(), d.detach(), g64, cpl)
    if fault == "missing_1e-10":
        gf = gf + _no_eps_fault(f.detach(), zz.detach(), d.detach())
    from loss_ref import awp_integrate_bwd
    r.update(d_feat=gf, d_z=gz, d_rays_d=gd, E_d_rays_d=awp_integrate_bwd(np.asarray(feat), np.asarray(z), np.asarray(rays_d), np.asarray(g), eps=EPS)["E_d_rays_d"])
    return r


def integrate32(feat, z, rays_d, g):
    """torch float32 of the same as-written lines: out, d_feat, d_z, d_rays_d"""
    a = [torch.tensor(np.asarray(t), dtype=torch.float32).requires_grad_(True) for t in (feat, z, rays_d)]
    out = _scan_fwd(*a, as_written=True)
    grads = torch.autograd.grad((out * torch.tensor(np.asarray(g), dtype=torch.float32)).sum(), a, allow_unused=True) if out.requires_grad else [None] * 3
    gf, gz, gd = (torch.zeros_like(x) if v is None else v for v, x in zip(grads, a))
    return dict(out=out.detach(), d_feat=gf, d_z=gz, d_rays_d=gd)


# ---- the MAM's per-sample part ----------------------------------------------------------------------------------------------------
def mam_arm(P, S):
    return "fwd_r" if P <= 10 and S <= 128 else "fwd"


def _wave3(S):
    """the samples of the fourth wavefront's lane groups (group g = s mod 16 owns sample s, a wavefront four groups)"""
    return ((torch.arange(S) % 16) // 4 == 3)


def _mam_fwd(h4, ur, fault=None):
    """h4 [R, P, S, 64], ur [R, 64] (u, one copy per ray) -> alpha, beta [R, P, S], h_inter [R, P, 64], h_intra [R, S, 64]"""
    a = torch.einsum("rpsc,rc->rps", h4, ur)
    alpha = torch.softmax(a, -2 if fault == "alpha_softmax_over_p" else -1)
    beta = torch.softmax(a, -1 if fault == "beta_softmax_over_s" else -2)
    wa = alpha * (~_wave3(a.shape[-1])).to(a.dtype) if fault == "h_inter_misses_a_wavefront" else alpha
    return alpha, beta, torch.einsum("rps,rpsc->rpc", wa, h4), torch.einsum("rps,rpsc->rsc", beta, h4)


def _mam_bwd(h4, u, alpha, beta, hi, hs, gi, gs, fault=None):
    """the header of kernel_mam.hip: d logit = alpha (gA - cP) + beta (gB - cI), d h = alpha d_inter + beta d_intra + d logit u, d u = sum d logit h"""
    # gA - cP = d_inter[p] . (h[p,s] - h_inter[p]), gB - cI = d_intra[s] . (h[p,s] - h_intra[s]): one dot each, so that a single-sample row
    # (alpha = 1, h_inter = h) and a single sub-exposure (beta = 1) give the exact 0 the kernel gives (its gA and cP are the same dot)
    dA = torch.einsum("rpc,rpsc->rps", gi, h4 if fault == "cP_left_out" else h4 - hi[:, :, None, :])
    dB = torch.einsum("rsc,rpsc->rps", gs, h4 if fault == "cI_left_out" else h4 - hs[:, None, :, :])
    da = alpha * dA + beta * dB
    dh = alpha[..., None] * gi[:, :, None, :] + beta[..., None] * gs[:, None, :, :]
    if fault != "dlogit_u_left_out":
        dh = dh + da[..., None] * u
    dw = da * (~_wave3(da.shape[-1])).double() if fault == "d_u_misses_a_wavefront" else da
    return dh, torch.einsum("rps,rpsc->rc", dw, h4)


def _mam_bound(h4, u):
    R, P, S, _ = h4.shape
    a = h4 @ u
    E_a = 8 * (h4.abs() @ u.abs())

    def soft(axis, n_sum, n_div):
        x = a - a.amax(axis, keepdim=True)
        E_x = E_a + E_a.amax(axis, keepdim=True) + (2 + LOG2E_REL) * x.abs()
        ex = torch.exp(x)
        E_ex = ex * (E_x + 2) + FLUSH
        t = ex.sum(axis, keepdim=True)
        E_t = E_ex.sum(axis, keepdim=True) + n_sum * t
        w = ex / t
        return w, E_ex / t + w * E_t / t + n_div * w

    alpha, E_alpha = soft(-1, -(-S // 64) + 6, 1)
    beta, E_beta = soft(-2, P, 2)
    ta, tb = (alpha[..., None] * h4).abs(), (beta[..., None] * h4).abs()
    E_hi = (E_alpha[..., None] * h4.abs()).sum(2) + (-(-S // 16) + 5) * ta.sum(2) + FLUSH
    E_hs = (E_beta[..., None] * h4.abs()).sum(1) + P * tb.sum(1) + FLUSH
    return dict(E_alpha=E_alpha, E_beta=E_beta, E_h_inter=E_hi, E_h_intra=E_hs)


def mam_local64(h, u, R, P, S, g_inter=None, g_intra=None, fault=None):
    """h [R P, S, 64], u [64] float32 -> alpha, beta [R, P, S], h_inter [R, P, 64], h_intra [R, S, 64] and E_<name> (units of u);  with
    the upstream gradients g_inter [R, P, 64], g_intra [R, S, 64] also d_h [R P, S, 64] and the per-ray d_u [R, 64]"""
    h4, u64 = _t64(h).reshape(R, P, S, MAM_C), _t64(u)
    alpha, beta, hi, hs = _mam_fwd(h4, u64.expand(R, MAM_C), fault)
    r = dict(alpha=alpha, beta=beta, h_inter=hi, h_intra=hs, **_mam_bound(h4, u64))
    if g_inter is not None:
        dh, du = _mam_bwd(h4, u64, alpha, beta, hi, hs, _t64(g_inter), _t64(g_intra), fault)
        r.update(d_h=dh.reshape(R * P, S, MAM_C), d_u=du)
    return r


def _mam_autograd(h, u, R, P, S, g_inter, g_intra, dtype):
    h4 = torch.tensor(np.asarray(h), dtype=dtype).reshape(R, P, S, MAM_C).requires_grad_(True)
    ur = torch.tensor(np.asarray(u), dtype=dtype).expand(R, MAM_C).clone().requires_grad_(True)
    alpha, beta, hi, hs = _mam_fwd(h4, ur)
    loss = (hi * torch.tensor(np.asarray(g_inter), dtype=dtype)).sum() + (hs * torch.tensor(np.asarray(g_intra), dtype=dtype)).sum()
    dh, du = torch.autograd.grad(loss, [h4, ur])
    return dict(alpha=alpha.detach(), beta=beta.detach(), h_inter=hi.detach(), h_intra=hs.detach(), d_h=dh.reshape(R * P, S, MAM_C), d_u=du)


def mam_local32(h, u, R, P, S, g_inter, g_intra):
    """torch float32 (values and autograd) of the same reduced formulas"""
    return _mam_autograd(h, u, R, P, S, g_inter, g_intra, torch.float32)


def mam_local64_autograd(h, u, R, P, S, g_inter, g_intra):
    return _mam_autograd(h, u, R, P, S, g_inter, g_intra, torch.float64)


def mam_unreduced64(h, Wl, bl, v, R, P, S, g_inter32=None, g_intra32=None):
    """mam.py:72-74, 29-33 as written: the linear on every sample, the 1x1 conv logit, two softmaxes, two sums.  inter [R, 32, P], intra
    [R, 32, S];  with upstream gradients of those shapes also d h [R P, S, 64], d linear.weight and d line_conv_att.weight"""
    x, W, v64 = _t64(h, True), _t64(Wl, True), _t64(np.asarray(v).reshape(-1), True)
    cur = (x.reshape(R, P, S, MAM_C) @ W.t() + _t64(bl)).permute(0, 3, 1, 2)            # [R, 32, P, S]
    att = (cur * v64[None, :, None, None]).sum(1, keepdim=True)
    inter, intra = (cur * att.softmax(-1)).sum(-1), (cur * att.softmax(-2)).sum(-2)
    r = dict(inter=inter.detach(), intra=intra.detach())
    if g_inter32 is not None:
        r["d_h"], r["d_W"], r["d_v"] = torch.autograd.grad((inter * _t64(g_inter32)).sum() + (intra * _t64(g_intra32)).sum(), [x, W, v64])
    return r


def consumers64(h, u, z, rays_d, g_int, g_inter, g_intra, R, P, S, fault=None):
    """h_local's two consumers: d_h (the sum of the two shares; d_h_scan is the integration's), d_z [R P, S], d_rays_d [R P, 3]
    (+ E_d_rays_d), per-ray d_u [R, 64]"""
    sc = integrate64(h, z, rays_d, g=g_int, fault=fault if fault in SCAN_FAULTS else None)
    mm = mam_local64(h, u, R, P, S, g_inter, g_intra, fault=fault if fault in MAM_FAULTS else None)
    return dict(d_h=sc["d_feat"] + mm["d_h"], d_h_scan=sc["d_feat"], d_z=sc["d_z"], d_rays_d=sc["d_rays_d"], E_d_rays_d=sc["E_d_rays_d"], d_u=mm["d_u"])


# ---- structural mistakes the reference reproduces on request: name -> (family, the outputs it can move) -----------------------------------
SCAN_FAULTS = {
    "cumprod_over_samples": "cumprod along the sample axis instead of the channel axis",
    "q_inclusive_of_own_row": "Q inclusive of the row's own om (off by one row)",
    "q_exclusive_over_channels": "Q exclusive along the channels (off by one channel)",
    "last_alpha_not_zeroed": "the last sample's alpha not zeroed",
    "dist_without_norm": "dist without |d|",
    "missing_1e-10": "om without the + 1e-10 (shows on the saturated rays only: their backward divides by om)",
    "suffix_sum_includes_own_lane": "the backward's suffix sum inclusive instead of exclusive of the lane to the right",
    "lane_last_channel_dropped": "the last channel of a multi-channel lane dropped from Q",
    "padding_channels_in_product": "channels >= C read without the guard (the following row's floats) and entering the scans",
}
SCAN_BWD_FAULTS = ("suffix_sum_includes_own_lane", "padding_channels_in_product")
MAM_FAULTS = {
    "alpha_softmax_over_p": "alpha's softmax over the sub-exposures",
    "beta_softmax_over_s": "beta's softmax over the samples",
    "cP_left_out": "cP left out of the softmax backward",
    "cI_left_out": "cI left out of the softmax backward",
    "dlogit_u_left_out": "the d logit u term left out of d h",
    "h_inter_misses_a_wavefront": "one wavefront's quarter missing from h_inter",
    "d_u_misses_a_wavefront": "one wavefront's quarter missing from d u",
}
MAM_FWD_ONLY = ("alpha_softmax_over_p", "beta_softmax_over_s", "h_inter_misses_a_wavefront")      # the backward entries take alpha, beta as inputs
FAULTS = {**SCAN_FAULTS, **MAM_FAULTS}


def fault_reaches(fault, case):
    """whether the mistake can exist in the kernel arm the case runs"""
    e, arm = case["entry"], case["arm"]
    if fault in SCAN_FAULTS:
        if e == "mam":
            return False
        if fault == "missing_1e-10":
            return case["variant"] == "saturated"
        if fault == "lane_last_channel_dropped":
            return CPL[arm] > 1
        if fault == "padding_channels_in_product":
            return e == "scan" and case["C"] < 64 * CPL[arm]
        return True
    if e == "scan":
        return False
    return e == "mam" or fault not in MAM_FWD_ONLY


# ---- the case matrix ----------------------------------------------------------------------------------------------------------------
def _scan_case(arm, C, N, S, variant=None):
    return dict(id=f"scan-{arm}-C{C}-N{N}-S{S}" + (f"-{variant}" if variant else ""), entry="scan", arm=arm, C=C, N=N, S=S, variant=variant)


def _mam_case(arm, R, P, S, variant=None):
    return dict(id=f"mam-{arm}-R{R}-P{P}-S{S}" + (f"-{variant}" if variant else ""), entry="mam", arm=arm, R=R, P=P, S=S, variant=variant)


def _cases():
    out = []
    # k_awp_integrate_c64 / _bwd_c64: 16 rays per workgroup -- every N at S = 5, every S at N = 17
    out += [_scan_case("c64", 64, N, 5) for N in (1, 15, 16, 17, 33)]
    out += [_scan_case("c64", 64, 17, S) for S in (1, 2, 3, 4, 9, 128)]
    # k_awp_integrate<CPL> / _bwd<CPL>: 4 rays per workgroup -- the middle C: every N at S = 5, every S at N = 5; the edge Cs at three shapes
    for arm, Cs, Ss in (("cpl1", (1, 20, 63), (1, 2, 5, 8, 9, 33)), ("cpl2", (65, 127, 128), (1, 2, 3, 4, 5, 33)), ("cpl4", (129, 200, 256), (1, 2, 3, 4, 5, 33))):
        out += [_scan_case(arm, Cs[1], N, 5) for N in (1, 3, 4, 5)]
        out += [_scan_case(arm, Cs[1], 5, S) for S in Ss if S != 5]
        out += [_scan_case(arm, Cs[0], 3, Ss[-2]), _scan_case(arm, Cs[0], 1, 2), _scan_case(arm, Cs[2], 4, 33), _scan_case(arm, Cs[2], 5, 3), _scan_case(arm, Cs[2], 1, 1)]
    for arm, C, N, S in (("c64", 64, 17, 9), ("cpl1", 20, 5, 9), ("cpl2", 127, 5, 5), ("cpl4", 200, 5, 5)):
        out += [_scan_case(arm, C, N, S, v) for v in ("zero_dir", "repeat_z", "null_arms", "saturated")]
    for R, P, S in ((1, 1, 1), (2, 1, 33), (2, 7, 16), (2, 7, 17), (2, 10, 127), (3, 10, 128)):
        out.append(_mam_case("fwd_r", R, P, S))
    for R, P, S in ((2, 11, 128), (2, 10, 129), (2, 16, 1), (2, 3, 300), (1, 16, 512)):
        out.append(_mam_case("fwd", R, P, S))
    for arm, R, P, S in (("fwd_r", 2, 7, 17), ("fwd", 2, 11, 128)):
        out += [_mam_case(arm, R, P, S, "peaked"), _mam_case(arm, R, P, S, "flat")]
    for R, P, S in ((2, 3, 1), (2, 3, 2), (3, 10, 33), (2, 10, 129), (1, 16, 18), (1, 16, 512)):
        out.append(dict(id=f"fused-R{R}-P{P}-S{S}", entry="fused", arm="consumers", R=R, P=P, S=S, variant=None))
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
ARMS = {"scan": ("c64", "cpl1", "cpl2", "cpl4"), "mam": ("fwd_r", "fwd"), "fused": ("consumers",)}


def expected_arm(case):
    """the dispatch of the entries (kernel_awp_integrate.hip, kernel_mam.hip) restated from the sizes alone"""
    if case["entry"] == "scan":
        C = case["C"]
        return "c64" if C == 64 else "cpl1" if C <= 64 else "cpl2" if C <= 128 else "cpl4"
    if case["entry"] == "mam":
        return "fwd_r" if case["P"] <= 10 and case["S"] <= 128 else "fwd"
    return "consumers"                                                                  # one kernel


def max_fd(feat, z, rays_d):
    """max over samples and channels of f dist, per ray (float64)"""
    f, zz, d = (np.asarray(t, np.float64) for t in (feat, z, rays_d))
    if f.shape[1] < 2:
        return np.zeros(f.shape[0])
    dist = np.diff(zz, axis=-1) * np.linalg.norm(d, axis=-1)[:, None]
    return (f[:, :-1].max(-1) * dist).max(-1)


def _scan_inputs(rs, N, S, C, scale=True):
    feat = np.abs(rs.standard_normal((N, S, C)))
    if scale:
        feat = feat * rs.choice([0.05, 1.0, 8.0], size=(N, 1, 1))
    z = np.sort(rs.uniform(0, max(S, 2) / Z_PER_SAMPLE, (N, S)).astype(np.float32), -1)
    d = rs.standard_normal((N, 3)).astype(np.float32)
    return feat, z, d


def _condition(feat, z, d):
    """rays whose max f dist lies outside [FD_FLOOR, FD_CAP] are scaled to just inside it (a zero direction or S = 1 has no f dist at all)"""
    feat = feat.astype(np.float32)
    fd = max_fd(feat, z, d)
    for n in np.flatnonzero(fd > 0):
        if fd[n] > 0.97 * FD_CAP:
            feat[n] *= np.float32(0.95 * FD_CAP / fd[n])
        elif fd[n] < 1.03 * FD_FLOOR:
            feat[n] *= np.float32(1.05 * FD_FLOOR / fd[n])
    return feat


def make_inputs(case, draw=0):
    """the case's float32 inputs, seeded by its id (and the number of the draw, see reference()): |N(0, 1)| features with per-ray scales from {0.05, 1, 8}, sorted uniform z, N(0, 1)
    directions and upstream gradients.  z spans (0, S / 2), not (0, 1): alpha = fl(1 - e) carries u / (f dist) of relative error, the
    conditioning of the as-written float32 formula and of any float32 evaluation of it, so a ray whose f dist is ~1e-3 (scale 0.05 at
    S = 128 on a unit z range) cannot be within 1e-5 PER RAY; with a mean interval of 0.5 the scale-0.05 rays sit at f dist ~0.03, where
    torch float32 is within a tenth of the tolerance, and the scale-8 rays reach FD_CAP.  Rays outside [FD_FLOOR, FD_CAP] (a small |d|, a
    short interval at S = 2) are scaled to its edge.  The MAM's h = max(N(0, 1), 0) and u = W^T v as tests/test_gpu_awp.py draws them"""
    rs = np.random.RandomState((zlib.crc32(case["id"].encode()) + draw) & 0x7fffffff)
    v = case["variant"]
    if case["entry"] == "scan":
        N, S, C = case["N"], case["S"], case["C"]
        feat, z, d = _scan_inputs(rs, N, S, C)
        ray = min(1, N - 1)
        if v == "zero_dir":
            d[0] = 0.0
        if v == "repeat_z":
            z[ray, S // 2] = z[ray, S // 2 - 1]
        feat = _condition(feat, z, d)
        sat = []
        if v == "saturated":
            feat[ray] *= np.float32(1.5 * FD_SAT / max_fd(feat, z, d)[ray])
            sat = [ray]
        return dict(feat=feat, z=z, rays_d=d, g=rs.standard_normal((N, C)).astype(np.float32), sat=sat)
    R, P, S = case["R"], case["P"], case["S"]
    h = np.maximum(rs.standard_normal((R * P, S, MAM_C)), 0).astype(np.float32)
    Wl = (rs.standard_normal((32, MAM_C)) * 0.125).astype(np.float32)
    vv = (rs.standard_normal(32) * 0.5).astype(np.float32)
    u = (Wl.T @ vv).astype(np.float32)
    if v == "peaked":
        a = h.astype(np.float64) @ u.astype(np.float64)                                # the widest row reaches the spread, no row goes far beyond
        a = a[np.argmax(np.ptp(a, axis=-1))]
        u = (u * (1.05 * SPREAD / np.ptp(a))).astype(np.float32)
    if v == "flat":
        u = np.zeros_like(u)
    r = dict(h=h, u=u, g_inter=rs.standard_normal((R, P, MAM_C)).astype(np.float32), g_intra=rs.standard_normal((R, S, MAM_C)).astype(np.float32),
             prefill=rs.standard_normal((R * P, S, MAM_C)).astype(np.float32))
    if case["entry"] == "fused":
        _, z, d = _scan_inputs(rs, R * P, S, 1, scale=False)
        d[1] = 0.0                                                                      # one sub-exposure ray with a zero direction
        if S >= 3:
            z[2, S // 2] = z[2, S // 2 - 1]                                             # one repeated z in mid-row
        r["h"] = h = _condition(h, z, d)
        r.update(z=z, rays_d=d, g_int=rs.standard_normal((R * P, MAM_C)).astype(np.float32))
    return r


def float32_margins(case, x, r):
    """torch float32 of the same formulas against the float64 reference r, every figure as a fraction of what the input conditions allow:
    a forward output's error over its bound at factor 1 (K = 2 is asserted of the kernels), a backward output's per-ray error over a
    TENTH of its tolerance (the saturated rays excepted: their backward is held to finiteness)"""
    e, tol = case["entry"], TOL[case["entry"]]
    m = {}
    if e == "scan":
        N = case["N"]
        ok = np.ones(N, bool)
        ok[x["sat"]] = False
        lo = integrate32(x["feat"], x["z"], x["rays_d"], x["g"])
        m["out"] = bound_ratio(lo["out"], r["out"], r["E_out"]) * K
        m["d_feat"] = per_ray_rel(lo["d_feat"], r["d_feat"], N)[ok].max() / (tol / 10)
        m["d_z"] = per_ray_rel(lo["d_z"], r["d_z"], N)[ok].max() / (tol / 10)
        m["d_rays_d"] = rays_d_rel(lo["d_rays_d"], r["d_rays_d"], r["E_d_rays_d"], tol)[ok].max() / (tol / 10)
        return m
    R, P, S = case["R"], case["P"], case["S"]
    lo = mam_local32(x["h"], x["u"], R, P, S, x["g_inter"], x["g_intra"])
    m["d_u"] = per_ray_rel(lo["d_u"], r["d_u"], R).max() / (tol / 10)
    if e == "mam":
        for k in ("alpha", "beta", "h_inter", "h_intra"):
            m[k] = bound_ratio(lo[k], r[k], r["E_" + k]) * K
        m["d_h"] = per_ray_rel(lo["d_h"], r["d_h"], R * P).max() / (tol / 10)
        return m
    sc = integrate32(x["h"], x["z"], x["rays_d"], x["g_int"])
    m["d_h"] = per_ray_rel(sc["d_feat"] + lo["d_h"], r["d_h"], R * P).max() / (tol / 10)
    m["d_z"] = per_ray_rel(sc["d_z"], r["d_z"], R * P).max() / (tol / 10)
    m["d_rays_d"] = rays_d_rel(sc["d_rays_d"], r["d_rays_d"], r["E_d_rays_d"], tol).max() / (tol / 10)
    return m


MAX_DRAWS = 64


@functools.lru_cache(maxsize=None)
def reference(case_id, fault=None):
    """(inputs, float64 reference) of a case, computed once and shared; treat both as read-only.

    The inputs are drawn until they meet the input condition that makes a tolerance meaningful: torch float32 of the same formulas
    within a tenth of it on every ray (float32_margins <= 1).  That is a property of the draw, not of a kernel: d z and d u are
    cancelling sums over the channels (g has both signs, and the direct and the through-Q parts of d dist have opposite signs), so
    about one ray in thirty of the stated distributions has a float32 noise of 1e-6 ... 6e-6 of its own gradient.  x["draw"] is the
    number of the draw that was kept, x["f32"] its margins; tests/test_awp_local_ref.py asserts them again."""
    case = BY_ID[case_id]
    if fault is not None:
        x = reference(case_id)[0]
    else:
        for draw in range(MAX_DRAWS):
            x = make_inputs(case, draw)
            r = _reference(case, x, None)
            x["draw"], x["f32"] = draw, float32_margins(case, x, r)
            if max(x["f32"].values()) <= 1:
                return x, r
        raise AssertionError(f"{case_id}: no draw of {MAX_DRAWS} meets the float32 condition: {x['f32']}")
    return x, _reference(case, x, fault)


def _reference(case, x, fault):
    if case["entry"] == "scan":
        return integrate64(x["feat"], x["z"], x["rays_d"], x["g"], fault=fault)
    R, P, S = case["R"], case["P"], case["S"]
    if case["entry"] == "mam":
        return mam_local64(x["h"], x["u"], R, P, S, x["g_inter"], x["g_intra"], fault=fault)
    return consumers64(x["h"], x["u"], x["z"], x["rays_d"], x["g_int"], x["g_inter"], x["g_intra"], R, P, S, fault=fault)


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def _np64(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def bound_ratio(got, ref, E):
    """worst |got - ref| / (K u E): <= 1 passes (E in units of u; an exact 0 bound demands an exact result)"""
    got, ref, E = _np64(got), _np64(ref), _np64(E)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / (K * U * E))
    return float(np.nan_to_num(q, nan=np.inf).max()) if q.size else 0.0


def per_ray_rel(got, ref, rays):
    """relative L2 of every ray's slice [rays];  a ray whose reference is exactly 0 gives 0 if the result is exactly 0, else inf"""
    g, r = _np64(got).reshape(rays, -1), _np64(ref).reshape(rays, -1)
    num, den = np.linalg.norm(g - r, axis=1), np.linalg.norm(r, axis=1)
    num = np.where(np.isfinite(g).all(1), num, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num == 0, 0.0, np.inf))


def rays_d_rel(got, ref, E, tol):
    """per ray: max |got - ref| / max(max |ref|, K u max E / tol);  exactly 0 where the reference is"""
    g, r, E = _np64(got).reshape(-1, 3), _np64(ref).reshape(-1, 3), _np64(E).reshape(-1, 3)
    err = np.abs(g - r).max(1)
    err = np.where(np.isfinite(g).all(1), err, np.inf)
    rmax = np.abs(r).max(1)
    den = np.maximum(rmax, K * U * E.max(1) / tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rmax > 0, err / den, np.where(err == 0, 0.0, np.inf))
