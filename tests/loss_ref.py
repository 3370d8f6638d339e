"""float64 reference of the loss-side kernels (csrc/kernels_loss.hip; the AWP scan: csrc/kernel_awp_integrate.hip + awp_integrate.h): the sub-exposure weighted sum (rbk_weighted_sum,
blurmodel.py:112-127), the response curves (tonemapping.py:59-93, none / gamma / learn), the blur-loss partial sums (run_nerf.py:443-497) with
their hand-written backward for the curves the backward kernel is built for (none, gamma, learn + skip_learn), the event-loss partial sums
(run_nerf.py:518-570, events.py:260-284) with their hand-written backward incl. the 705-float parameter gradient, and the AWP consumer's
compositing scan AS WRITTEN in the reference (awp.py:49-77: the cumprod runs along the CHANNEL axis of the previous sample's row) with its
hand-written backward.  Every function
returns each output next to a first-order error bound E in units of u = 2^-24, built from the kernels' own operation counts.  Test
infrastructure only.

The reference's `- alpha + (1. + 1e-10)` (awp.py:72): in float32 1.f + 1e-10f == 1.f, so on float32 tensors the term is a no-op and the
forward kernels' om is fl(1 - alpha).  The float64 truth therefore carries no 1e-10; `eps` restores it (tests/test_loss_ref.py pins G15 with
both).  The BACKWARD kernels use om = fl(e + 1e-10f), which is live below e ~ 1e-3: their bound carries the absolute 1e-10 per factor of Q.

Error model (units of u; a rounding is <= u relative; a product of k factors takes k - 1 roundings in ANY association, a sum's error is
(roundings along the longest path) x sum |terms|):
  weighted_sum   s += x ccw, P steps (an FMA or a product and an add)         sum_p |x ccw| (1 + P)
  dist           fl(fl(z1 - z0) norm): dz 1, the float32 norm 2.5 (three __fmul_rn, two __fadd_rn: 1.5 under the root, halved, + sqrtf's
                 own + the products'), the product 1                         5 |dist|  (composite_ref.py's figure)
  x = f dist     the product 1; exp_fast scales by float32(log2 e) (0.22 u off the real log2 e) and rounds: 1.25
                                                                             E_x = |f| E_dist + 2.25 |x| = 7.25 |x|
  e = exp2(.)    v_exp_f32, 1 ulp = 2 u                                      E_e = e (E_x + 2)
  alpha = 1 - e  E_alpha = E_e + |alpha|;  forward om = fl(1 - alpha): E_om = E_alpha + |om| (~u ABSOLUTE once alpha -> 1, and exactly
                 0 when e < 2^-25);  backward om = fl(e + 1e-10f): E_om = E_e + |om| + |1e-10 - eps| / u
  Q[s+1, c]      prod_{c' <= c} om[s, c']: lane-local products, the DPP scan and the per-channel `excl *= om` multiply every factor in
                 exactly once (products with 1.f are exact), so one rounding per factor:
                 E_Q(c + 1) = E_Q(c) om^ + Q^(c) E_om(c) + Q^(c + 1),  with om^ = |om| + u E_om and Q^ = prod om^ the UPPER magnitudes: next to
                 an opaque channel the error of om is as large as om itself, and the product of two such errors is not second order
  out[c]         t = fl(fl(alpha Q) f): |f| (Q^ E_alpha + |alpha| E_Q) + 2 |t|;  S sequential adds: sum_s E_t + S sum_s |t|
Backward (d out = g;  H[s, c] = g a[s, c] f[s, c];  through[s, c] = sum_{c'' >= c} H[s+1, c''] Q[s+1, c''] / om[s, c], which the reference
evaluates without the division as P[s, c] T[s, c], P the exclusive prefix product of om[s, :] and T_c = H[s+1, c] + om[s, c+1] T_(c+1)):
  G = g a' f' Q'          three products                                      |g f'| (Q^ E_a' + |a'| E_Q') + 3 |G|
  suffix sums of G        generic: lane sum (CPL - 1), 6 DPP adds, both for `total` and for the inclusive prefix, their difference (1) and
                          CPL adds back: 3 CPL + 11 roundings, each bounded by the WHOLE row's sum |G| (total - prefix cancels);
                          c64: lane sum (3), 4 DPP adds to the right, `- lsum` (1), 4 adds: 12 roundings on the sum |G| of this lane's
                          channels and those to its right
  through = sfx / om      (E_sfx + |sfx| E_om) / om_k + n_div |through|, om_k = e + 1e-10 the kernel's divisor; n_div = 1 (IEEE
                          division), 3 in c64 (v_rcp_f32 1 ulp = 2 u, and the product)
  ga = g Q f - through    |g f| E_Q + 2 |g Q^ f| + E_through + |g Q f| + |through|
  d f = g Q a + ga dist e |g| (Q^ E_a + |a| E_Q) + 2 |g Q a| + |dist e| E_ga + ga^ (e E_dist + |dist| E_e) + 2 |ga dist e| + both terms once more
  d dist = sum_c ga f e   |f e| E_ga + ga^ |f| E_e + 2 |.| per term; CPL + 6 adds (c64: 3 + 4) on sum |terms|
  d z[s]                  p[s] = ddist[s] norm: norm E_ddist + 3.5 |p|;  d z[s] = p[s-1] - p[s]: both bounds + |p[s-1]| + |p[s]|
  d rays_d                dnorm = sum_s ddist dz (|dz| E_ddist + 2 |.| per term, S adds);  dnorm d / |d|: |d| / |d| (E_dnorm + 5 |dnorm|); 0 at |d| = 0
Blur loss (per lane = pixel x channel: a = sum_p rgb_p w1 etc., P steps of FMA; the squared error; block_sum = 6 shuffles + nw LDS adds; one
float atomicAdd per 64-lane block in arbitrary order):
  a, b, c                 sum_p |f w| (1 + P)
  crf: none               exact;  gamma: powf(v, 1/2.2), POW_ULP ulp = 2 POW_ULP u, conditioned by (1/g) v^(1/g - 1) on E_v;  learn with
                          skip_learn: identity (tonemapping.py:64-68: the gamma branch is `map_type == gamma` only)
  se = (crf - t)^2        d = crf - t: E_crf + |d|;  se: 2 |d| E_d + |se|
  partial[k]              sum E_se + (6 + 1 + nblocks) sum |se| (+ the value handed in, exact);  partial[5] = 3 R exactly (integers < 2^24)
  backward                da = 2 g (crf(a) - t) crf'(a): |2 g| (|crf'| E_d + |d| E_crf') + 3 |da|;  crf' = (1/g) powf(a, 1/g - 1): 2 POW_ULP + 1
                          relative and |(1/g - 1)| E_a / |a| through the argument;  d rgb_p = da w1 + dc w2 (+ the pts0 term on p = 0): each
                          product's bound + one rounding per add;  d w1[q] = three atomicAdds of da f + db f0 in arbitrary order: each
                          term's bound + 3 sum |terms|
Response curves with live weights (crf_apply: 1 + E -> 16 -> 16 -> 16 -> 1, y = sigmoid(0.1 s + v)) and evd_crf_forward:
  a layer                 s_j = b_j + sum_k w_jk h_k as fan-in fmaf's, each rounding a partial sum bounded by sum |w h| + |b|:
                          fan_in (sum_k |w_jk h_k| + |b_j|) + sum_k |w_jk| E_h_k; fan-in 1 + E in layer 0 (the padded columns multiply 0), 16 after
  ReLU                    a discrete decision: E_h = E_s where s > 0, and the INPUTS ARE CHOSEN so that no pre-activation lies inside K u of its
                          own bound (`safe`; the generators of the tests drop the rows that do and assert that they are at most 5 %)
  y                       t = fl(fl(s 0.1f) + v): 0.1 E_s + 1.5 |0.1 s| (float32(0.1) is 0.4 u off) + E_v + |t|;  expf 2 u (composite_ref.py's
                          figure), 1 + e, the IEEE division: y (1 - y) (E_t + 2) + 2 y
  luma                    three products by a float32 coefficient (its rounding 0.5 + the product 1) and two adds: sum c E_y + 3.5 sum |c y|;
                          avg: two adds and the division: sum E_y / 3 + sum |y|
Event loss (16 lanes per event; block_sum = 6 shuffles + 4 LDS adds; one atomicAdd per 16-event block in arbitrary order):
  lg = logf(lum + 1e-5f)  the add: E_lum + |arg|;  logf LOG_ULP ulp, conditioned by 1 / arg: 2 LOG_ULP |lg| + E_arg / arg
  pred - bii              pred = lg_end - lg_start: both bounds + |pred|;  bii = fl(fl(tn cn) + fl(tp cp)): |tn cn| + |tp cp| + |bii|;  d: + |d|
  partial[0], [1]         t = d d w: 2 |d| w E_d + 2 |t|;  sum E_t + (6 + 4 + nblocks) sum |t|;  partial[2] = sum w: exact for w = 1 (a count)
  backward                d_lg = +-2 g w d: |2 g w| E_d + 3 |d_lg|;  d_lum = d_lg / arg: E_d_lg / arg + |d_lum| (E_arg / arg + 1);  d_v = d_lum coef: + 1.5 |d_v|
                          none: d_x = d_v;  gamma: d_x = d_v (1/g) powf(x, 1/g - 1): |crf'| E_d_v + (2 POW_ULP + 2) |d_x|
                          learn: dz = d_v y (1 - y) with y rounded: |y (1 - y)| E_d_v + |d_v| (E_y (|1 - y| + |y|) + 2 |y (1 - y)|) + |dz|;  ds = 0.1f dz;
                          dh3 = mask ds w3;  dh2 = mask W2^T dh3, dh1 = mask W1^T dh2, d in0 = w0[:, 0] . dh1: 16 fmaf's each, as the forward layers;
                          d_x = dz + d in0
  d_params                per-lane products (dh1 in, dh2 h1, dh3 h2, ds h3, and the dh / ds themselves for the biases): both factors' bounds + 1;
                          wave_sum_dpp (4 DPP adds + 3), one LDS atomic per wavefront (4), one global atomic per block, all in arbitrary order:
                          sum E_c + (7 + 4 + nblocks) sum |c|.  Columns 3..7 of the w0 gradient are exactly 0
POW_ULP, LOG_ULP: powf and logf have no figure in the project, so their constants are measured (tools/measure_pow_log_ulp.py: float32 torch.pow /
torch.log on the MI355X against float64, 2^25 points per function, log-uniform and linear): pow(x, 1/2.2) 1.3128 ulp and pow(x, 1/2.2 - 1)
1.3019 ulp on [1e-4, 4], log(x) 1.8842 ulp on [1e-5, 4] (and exp(-x) 0.8512 ulp on [1e-3, 80], inside the 1 ulp = 2 u used for expf).  The
constants are those figures rounded up to an integer plus 1 (the kernels call the device library directly and need not hit the same worst
input): POW_ULP = 3, LOG_ULP = 3.
"""
import numpy as np
import torch

U = 2.0 ** -24
LOG2E_REL = 0.25            # float32(log2 e) is 0.22 u off log2 e
POW_ULP = 3                 # ceil(1.3128) + 1 (measured on the MI355X, see the docstring)
LOG_ULP = 3                 # ceil(1.8842) + 1
GAMMA = 2.2


def _f64(t, dev=None):
    t = torch.as_tensor(t)
    return t.to(device=dev if dev is not None else t.device, dtype=torch.float64)


# ---- evd_weighted_sum -----------------------------------------------------------------------------------------------------------
def weighted_sum(x, ccw):
    """x [R, P, C], ccw [R, P] -> (sum_p x ccw [R, C], E)"""
    x = _f64(x)
    w = _f64(ccw, x.device)
    P = x.shape[1]
    t = x * w[..., None]
    return t.sum(1), (1 + P) * t.abs().sum(1)


# ---- the AWP consumer's compositing scan ----------------------------------------------------------------------------------------
def awp_form(C):
    """the kernel the entries dispatch for C channels: channels per lane, roundings of the suffix sum / the d dist sum / the division"""
    if C == 64:
        return dict(name="c64", cpl=4, n_sfx=12, n_dd=7, n_div=3, right_only=True)
    cpl = 1 if C < 64 else 2 if C <= 128 else 4
    return dict(name=f"<{cpl}>", cpl=cpl, n_sfx=3 * cpl + 11, n_dd=cpl + 6, n_div=1, right_only=False)


def _awp_common(feat, z, rays_d, eps, backward):
    f = _f64(feat)
    dev = f.device
    N, S, C = f.shape
    z = _f64(z, dev)
    d = _f64(rays_d, dev)[:, :3]
    norm = d.norm(dim=-1)
    dz = z[:, 1:] - z[:, :-1]
    dist = torch.cat([dz * norm[:, None], torch.zeros_like(z[:, :1])], 1)            # [N, S], the last row has no interval
    E_dist = 5 * dist.abs()
    x = f * dist[..., None]
    E_x = f.abs() * E_dist[..., None] + (2 + LOG2E_REL) * x.abs()
    live = torch.ones((1, S, 1), dtype=torch.float64, device=dev)
    live[:, -1] = 0                                                                    # awp.py:67: zeros appended, alpha[S - 1] = 0
    e = torch.exp(-x)
    E_e = e * (E_x + 2) * live
    e = torch.where(live > 0, e, torch.ones_like(e))
    a = (1 - e) * live
    E_a = (E_e + a.abs()) * live
    om = e + eps
    if backward:
        E_om = E_e + om.abs() + abs(1e-10 - eps) / U
        om_k = e + 1e-10
    else:
        E_om = E_a + om.abs()
        om_k = om
    om_hi = om.abs() + U * E_om
    # Q of row s + 1 from om of row s; Q[0] = 1 exactly
    one = torch.ones_like(f[:, :1])
    P_excl = torch.cat([torch.ones_like(om[..., :1]), torch.cumprod(om, -1)[..., :-1]], -1)      # prod_{c' < c} om[s, c']
    Qn = P_excl * om
    Qn_hi = torch.cumprod(om_hi, -1)
    E_Qn = torch.empty_like(Qn)
    run = torch.zeros_like(om[..., 0])
    prev_hi = torch.ones_like(run)
    for c in range(C):
        run = run * om_hi[..., c] + prev_hi * E_om[..., c] + (Qn_hi[..., c] if c > 0 else 0.0)     # the first factor multiplies 1.f: exact
        E_Qn[..., c] = run
        prev_hi = Qn_hi[..., c]
    Q = torch.cat([one, Qn[:, :-1]], 1)
    Q_hi = torch.cat([one, Qn_hi[:, :-1]], 1)
    E_Q = torch.cat([torch.zeros_like(one), E_Qn[:, :-1]], 1)
    return dict(f=f, z=z, d=d, norm=norm, dz=dz, dist=dist, E_dist=E_dist, e=e, E_e=E_e, a=a, E_a=E_a, om=om, E_om=E_om, om_k=om_k,
                P_excl=P_excl, Q=Q, Q_hi=Q_hi, E_Q=E_Q, live=live)


def awp_integrate(feat, z, rays_d, eps=0.0):
    """feat [N, S, C], z [N, S], rays_d [N, 3] -> (out [N, C], E)"""
    q = _awp_common(feat, z, rays_d, eps, backward=False)
    f, S = q["f"], q["f"].shape[1]
    t = q["a"] * q["Q"] * f
    E_t = f.abs() * (q["Q_hi"] * q["E_a"] + q["a"].abs() * q["E_Q"]) + 2 * t.abs()
    return t.sum(1), E_t.sum(1) + S * t.abs().sum(1)


def awp_integrate_autograd(feat, z, rays_d, eps=0.0):
    """awp.py:58-75 as plain torch ops (float64 autograd)"""
    dists = (z[..., 1:] - z[..., :-1]) * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = -torch.exp(-feat[..., :-1, :] * dists[..., None]) + 1
    alpha = torch.cat([alpha, torch.zeros_like(alpha[:, 0:1])], dim=-2)
    ones = torch.ones((alpha.shape[0], 1, alpha.shape[-1]), dtype=feat.dtype, device=feat.device)
    w = alpha * torch.cumprod(torch.cat([ones, -alpha + (1. + eps)], -2), -1)[:, :-1, :]
    return torch.sum(w * feat, dim=-2)


def _rev_cumsum(t):
    return t.flip(-1).cumsum(-1).flip(-1)


def awp_integrate_bwd(feat, z, rays_d, d_out, eps=0.0):
    """hand-written float64 backward: d_feat [N, S, C], d_z [N, S], d_rays_d [N, 3] and E_<name>, for the kernel form the entry dispatches"""
    q = _awp_common(feat, z, rays_d, eps, backward=True)
    f, e, a, om, Q, Q_hi, E_Q = q["f"], q["e"], q["a"], q["om"], q["Q"], q["Q_hi"], q["E_Q"]
    N, S, C = f.shape
    fm = awp_form(C)
    dev = f.device
    g = _f64(d_out, dev)[:, None, :]
    dist, E_dist, E_e, E_a, E_om, om_k = q["dist"][..., None], q["E_dist"][..., None], q["E_e"], q["E_a"], q["E_om"], q["om_k"]
    zrow = torch.zeros_like(f[:, :1])
    nx = lambda t: torch.cat([t[:, 1:], zrow], 1)                                     # the next sample row's quantity at row s
    H = nx(g * a * f)                                                                  # H[s + 1, c] seen from row s
    T = torch.empty_like(f)
    run = torch.zeros_like(f[..., 0])
    for c in range(C - 1, -1, -1):
        run = H[..., c] + (om[..., c + 1] * run if c + 1 < C else 0.0)
        T[..., c] = run
    through = q["P_excl"] * T
    # the kernel's path to the same number: G, its suffix sums, the division
    Gk = H * nx(Q)
    E_G = (g * nx(f)).abs() * (nx(Q_hi) * nx(E_a) + nx(a).abs() * nx(E_Q)) + 3 * (H.abs() * nx(Q_hi))
    G_hi = H.abs() * nx(Q_hi)
    if fm["right_only"]:
        lane0 = (torch.arange(C, device=dev) // 4) * 4
        reach = lambda t: _rev_cumsum(t)[..., lane0]
    else:
        reach = lambda t: t.sum(-1, keepdim=True).expand_as(t)
    sfx = _rev_cumsum(Gk)
    E_sfx = reach(E_G) + fm["n_sfx"] * reach(G_hi)
    E_through = (E_sfx + sfx.abs() * E_om) / om_k + fm["n_div"] * through.abs()
    direct = g * Q * f
    ga = direct - through
    E_ga = (g * f).abs() * E_Q + 2 * (g * f).abs() * Q_hi + E_through + direct.abs() + through.abs()
    ga_hi = ga.abs() + U * E_ga
    t1 = g * Q * a
    t2 = ga * dist * e
    d_feat = (t1 + t2) * q["live"]
    E_d_feat = (g.abs() * (Q_hi * E_a + a.abs() * E_Q) + 2 * t1.abs() + (dist * e).abs() * E_ga + ga_hi * (e * E_dist + dist.abs() * E_e)
                + 2 * t2.abs() + t1.abs() + t2.abs()) * q["live"]
    term = ga * f * e * q["live"]
    E_term = ((f * e).abs() * E_ga + ga_hi * f.abs() * E_e + 2 * term.abs()) * q["live"]
    ddist = term.sum(-1)                                                               # [N, S], 0 on the last row
    E_ddist = E_term.sum(-1) + fm["n_dd"] * term.abs().sum(-1)
    norm = q["norm"][:, None]
    p = ddist * norm
    E_p = norm * E_ddist + 3.5 * p.abs()
    z1 = torch.zeros_like(p[:, :1])
    d_z = torch.cat([z1, p[:, :-1]], 1) - p
    E_d_z = torch.cat([z1, E_p[:, :-1]], 1) + E_p + torch.cat([z1, p[:, :-1].abs()], 1) + p.abs()
    qq = ddist[:, :-1] * q["dz"]
    dnorm = qq.sum(1)
    E_dnorm = (q["dz"].abs() * E_ddist[:, :-1] + 2 * qq.abs()).sum(1) + S * qq.abs().sum(1)
    nz = q["norm"] > 0
    inv = torch.where(nz, 1 / torch.where(nz, q["norm"], torch.ones_like(q["norm"])), torch.zeros_like(q["norm"]))[:, None]
    d_rd = dnorm[:, None] * q["d"] * inv
    E_d_rd = q["d"].abs() * inv * (E_dnorm + 5 * dnorm.abs())[:, None]
    return dict(d_feat=d_feat, E_d_feat=E_d_feat, d_z=d_z, E_d_z=E_d_z, d_rays_d=d_rd, E_d_rays_d=E_d_rd)


# ---- blur loss ------------------------------------------------------------------------------------------------------------------
def crf_simple(v, E_v, map_type, skip_learn=False, params=None, safe=None):
    """the response curves of the image branch on a computed value v with bound E_v: (crf(v), E, crf'(v), E of crf').  A live learn CRF
    (forward only: crf' is NaN) goes through mlp() and clears the rows of `safe` that have a pre-activation inside its bound"""
    if map_type == "gamma":
        ig = float(np.float32(1.0 / float(np.float32(GAMMA))))
        y = torch.pow(v, ig)
        dy = ig * torch.pow(v, ig - 1.0)
        E_y = 2 * POW_ULP * y.abs() + torch.where(E_v > 0, dy.abs() * E_v, torch.zeros_like(E_v))        # an exact 0 stays exact
        # crf' = fl(ig powf(a, fl(ig - 1))): the exponent's rounding moves the power by u |ig - 1| |ln v|, powf, the product; the argument
        E_dy = dy.abs() * (2 * POW_ULP + 1 + abs(ig - 1.0) * torch.log(v).abs() + abs(ig - 1.0) * E_v / v.abs())
        return y, E_y, dy, E_dy
    if map_type == "learn" and not skip_learn:
        m = mlp(unpack_params(params, v.device), v, E_v, None)
        if safe is not None:
            safe &= m["safe"].all(-1)
        nan = torch.full_like(v, float("nan"))
        return m["y"], m["E_y"], nan, nan
    return v, E_v, torch.ones_like(v), torch.zeros_like(v)


def _blur_common(rgb_p, rgb0_p, w1, w2, map_type, skip_learn, params=None):
    f = _f64(rgb_p)
    dev = f.device
    R, P, _ = f.shape
    wa = _f64(w1, dev)[..., None]
    out = dict(f=f, wa=wa, R=R, P=P, dev=dev, safe=torch.ones(R, dtype=torch.bool, device=dev))

    def mix(x, w):
        t = x * w
        v, E = t.sum(1), (1 + P) * t.abs().sum(1)
        return (v, E) + crf_simple(v, E, map_type, skip_learn, params, out["safe"])
    out["a"] = mix(f, wa)
    if rgb0_p is not None:
        out["f0"] = _f64(rgb0_p, dev)
        out["b"] = mix(out["f0"], wa)
    if w2 is not None:
        out["wb"] = _f64(w2, dev)[..., None]
        out["c"] = mix(f, out["wb"])
    return out


def _se(y, E_y, t):
    d = y - t
    E_d = E_y + d.abs()
    se = d * d
    return d, E_d, se, 2 * d.abs() * E_d + se.abs()


def blur_loss(rgb_p, w1, tgt, rgb0_p=None, w2=None, tgt0=None, map_type="none", skip_learn=False, partial0=None, params=None):
    """rgb_p [R, P, 3], w1 / w2 [R, P], tgt / tgt0 [R, 3] -> partial [6] + E, the colour outputs rgb, rgb1, rgb_awp [R, 3] + E, and `safe` [R]
    (a live learn CRF: no pre-activation of the pixel's evaluations inside its bound)"""
    q = _blur_common(rgb_p, rgb0_p, w1, w2, map_type, skip_learn, params)
    dev, R = q["dev"], q["R"]
    t = _f64(tgt, dev)
    nblocks = -(-3 * R // 64)
    n_red = 6 + 1 + nblocks
    part = torch.zeros(6, dtype=torch.float64, device=dev)
    E_part = torch.zeros(6, dtype=torch.float64, device=dev)

    def put(k, y, E_y, tt):
        _, _, se, E_se = _se(y, E_y, tt)
        part[k] = se.sum()
        E_part[k] = E_se.sum() + n_red * se.abs().sum()
    put(0, q["a"][2], q["a"][3], t)
    out = dict(rgb=q["a"][0], E_rgb=q["a"][1])
    if "b" in q:
        put(1, q["b"][2], q["b"][3], t)
        out.update(rgb1=q["b"][0], E_rgb1=q["b"][1])
    if "c" in q:
        put(2, q["c"][2], q["c"][3], t)
        out.update(rgb_awp=q["c"][0], E_rgb_awp=q["c"][1])
    if tgt0 is not None:
        t0 = _f64(tgt0, dev)
        y = crf_simple(q["f"][:, 0], torch.zeros_like(t0), map_type, skip_learn, params, q["safe"])
        put(3, y[0], y[1], t0)
        if "f0" in q:
            y = crf_simple(q["f0"][:, 0], torch.zeros_like(t0), map_type, skip_learn, params, q["safe"])
            put(4, y[0], y[1], t0)
    part[5] = 3 * R
    if partial0 is not None:
        p0 = _f64(partial0, dev)
        part = part + p0
        E_part = E_part + part.abs() + n_red * p0.abs()          # the atomics land on the value handed in, in any order
    out.update(partial=part, E_partial=E_part, safe=q["safe"])
    return out


def blur_loss_autograd(rgb_p, w1, tgt, rgb0_p=None, w2=None, tgt0=None, map_type="none"):
    """the five squared-error sums as plain torch ops (float64 autograd); absent terms are 0"""
    crf = (lambda v: torch.pow(v, float(np.float32(1.0 / float(np.float32(GAMMA)))))) if map_type == "gamma" else (lambda v: v)
    zero = rgb_p.sum() * 0
    mix = lambda x, w: (x * w[..., None]).sum(1)
    p = [((crf(mix(rgb_p, w1)) - tgt) ** 2).sum(), zero, zero, zero, zero]
    if rgb0_p is not None:
        p[1] = ((crf(mix(rgb0_p, w1)) - tgt) ** 2).sum()
    if w2 is not None:
        p[2] = ((crf(mix(rgb_p, w2)) - tgt) ** 2).sum()
    if tgt0 is not None:
        p[3] = ((crf(rgb_p[:, 0]) - tgt0) ** 2).sum()
        if rgb0_p is not None:
            p[4] = ((crf(rgb0_p[:, 0]) - tgt0) ** 2).sum()
    return p


def blur_loss_bwd(rgb_p, w1, tgt, g, rgb0_p=None, w2=None, tgt0=None, map_type="none", skip_learn=False):
    """hand-written backward of g[0..4] . partial[0..4]: d_rgb_p, d_rgb0_p [R, P, 3], d_w1, d_w2 [R, P] (None where the kernel writes
    nothing) and their bounds"""
    q = _blur_common(rgb_p, rgb0_p, w1, w2, map_type, skip_learn)
    dev, f, wa = q["dev"], q["f"], q["wa"]
    t = _f64(tgt, dev)
    g = [float(v) for v in g]

    def head(k, y, E_y, dy, E_dy, tt):
        """2 g (crf - t) crf' and its bound"""
        d, E_d, _, _ = _se(y, E_y, tt)
        v = 2 * g[k] * d * dy
        return v, abs(2 * g[k]) * (dy.abs() * E_d + d.abs() * E_dy) + 3 * v.abs()
    da, E_da = head(0, *q["a"][2:], t)
    da, E_da = da[:, None], E_da[:, None]
    dr, E_dr = da * wa, E_da * wa.abs() + (da * wa).abs()
    dw1_terms = [(da * f, E_da * f.abs() + (da * f).abs())]
    out = {}
    if "c" in q:
        dc, E_dc = head(2, *q["c"][2:], t)
        dc, E_dc = dc[:, None], E_dc[:, None]
        u2 = dc * q["wb"]
        E_dr = E_dr + E_dc * q["wb"].abs() + u2.abs() + (dr.abs() + u2.abs())
        dr = dr + u2
        tw = dc * f
        out["d_w2"] = tw.sum(-1)
        out["E_d_w2"] = (E_dc * f.abs() + tw.abs()).sum(-1) + 3 * tw.abs().sum(-1)
    if "b" in q:
        f0 = q["f0"]
        db, E_db = head(1, *q["b"][2:], t)
        db, E_db = db[:, None], E_db[:, None]
        dr0, E_dr0 = db * wa, E_db * wa.abs() + (db * wa).abs()
        dw1_terms.append((db * f0, E_db * f0.abs() + (db * f0).abs()))
    if tgt0 is not None:
        t0 = _f64(tgt0, dev)
        y = crf_simple(f[:, 0], torch.zeros_like(t0), map_type, skip_learn)
        d3, E_d3 = head(3, *y, t0)
        E_dr[:, 0] = E_dr[:, 0] + E_d3 + dr[:, 0].abs() + d3.abs()
        dr = dr.clone()
        dr[:, 0] = dr[:, 0] + d3
        if "b" in q:
            y = crf_simple(q["f0"][:, 0], torch.zeros_like(t0), map_type, skip_learn)
            d4, E_d4 = head(4, *y, t0)
            E_dr0[:, 0] = E_dr0[:, 0] + E_d4 + dr0[:, 0].abs() + d4.abs()
            dr0 = dr0.clone()
            dr0[:, 0] = dr0[:, 0] + d4
    out.update(d_rgb_p=dr, E_d_rgb_p=E_dr)
    if "b" in q:
        out.update(d_rgb0_p=dr0, E_d_rgb0_p=E_dr0)
    tw = sum(v for v, _ in dw1_terms)                                                 # per lane da f + db f0, then three atomics
    E_tw = sum(E for _, E in dw1_terms) + sum(v.abs() for v, _ in dw1_terms) * (len(dw1_terms) - 1)
    out["d_w1"] = tw.sum(-1)
    out["E_d_w1"] = E_tw.sum(-1) + 3 * tw.abs().sum(-1)
    return out


# ---- the response curves with live weights, evd_crf_forward ---------------------------------------------------------------------------
CRF_MAX_IN = 8
CRF_NPARAM = 16 * CRF_MAX_IN + 16 + 256 + 16 + 256 + 16 + 16 + 1
LUMA = {"rec601": (0.299, 0.587, 0.114), "rec709": (0.2126, 0.7152, 0.0722)}
LUMA_CODE = {-1: None, 0: "rec601", 1: "rec709", 2: "avg"}
IG32 = float(np.float32(1.0 / float(np.float32(GAMMA))))          # evd_crf_create: (float)(1.0 / (double)gamma)
IG1_32 = float(np.float32(np.float32(IG32) - np.float32(1.0)))    # inv_gamma - 1.f in float32


def pack_params(sd, extra_features, prefix=""):
    """the reference's linear.{0,2,4,6}.{weight,bias} -> the flat layout of evd_event_loss_bwd / evd_crf_get_params (w0 rows padded to 8)"""
    nin = 1 + extra_features
    w0 = np.zeros((16, CRF_MAX_IN), np.float32)
    w0[:, :nin] = np.asarray(sd[f"{prefix}linear.0.weight"], np.float32)
    parts = [w0, sd[f"{prefix}linear.0.bias"], sd[f"{prefix}linear.2.weight"], sd[f"{prefix}linear.2.bias"], sd[f"{prefix}linear.4.weight"],
             sd[f"{prefix}linear.4.bias"], sd[f"{prefix}linear.6.weight"], sd[f"{prefix}linear.6.bias"]]
    return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts])


def unpack_params(flat, dev):
    p = _f64(flat, dev)
    o = 0
    out = {}
    for k, shp in (("w0", (16, CRF_MAX_IN)), ("b0", (16,)), ("w1", (16, 16)), ("b1", (16,)), ("w2", (16, 16)), ("b2", (16,)), ("w3", (16,)), ("b3", ())):
        n = int(np.prod(shp)) if shp else 1
        out[k] = p[o:o + n].reshape(shp)
        o += n
    return out


def _layer(w, b, h, E_h, fan):
    """s = b + sum_k w[j, k] h[k] as `fan` FMAs, each rounding a partial sum that sum |w h| + |b| bounds"""
    s = h @ w.T + b
    mag = h.abs() @ w.abs().T + b.abs()
    return s, fan * mag + E_h @ w.abs().T


def mlp(params, v, E_v, feat):
    """the 1 + E -> 16 -> 16 -> 16 -> 1 network and the sigmoid of (0.1 s + v) on v [...], feat [..., <= 7] or None.  Returns a dict with the
    value y, its bound, the hidden layers, their pre-activations' bounds and `safe`: no pre-activation inside K u of its own bound."""
    p = params
    inp = torch.zeros(v.shape + (CRF_MAX_IN,), dtype=torch.float64, device=v.device)
    E_in = torch.zeros_like(inp)
    inp[..., 0], E_in[..., 0] = v, E_v
    nf = 0
    if feat is not None:
        nf = feat.shape[-1]
        inp[..., 1:1 + nf] = feat
    s1, E_s1 = _layer(p["w0"], p["b0"], inp, E_in, 1 + nf)
    h1, E_h1 = torch.relu(s1), E_s1 * (s1 > 0)
    s2, E_s2 = _layer(p["w1"], p["b1"], h1, E_h1, 16)
    h2, E_h2 = torch.relu(s2), E_s2 * (s2 > 0)
    s3, E_s3 = _layer(p["w2"], p["b2"], h2, E_h2, 16)
    h3, E_h3 = torch.relu(s3), E_s3 * (s3 > 0)
    s = h3 @ p["w3"] + p["b3"]
    E_s = 16 * (h3.abs() @ p["w3"].abs() + p["b3"].abs()) + E_h3 @ p["w3"].abs()
    t = 0.1 * s + v                                  # fl(s 0.1f) + v or one FMA; float32(0.1) is 0.4 u off 0.1
    E_t = 0.1 * E_s + 1.5 * (0.1 * s).abs() + E_v + t.abs()
    y = torch.sigmoid(t)
    E_y = y * (1 - y) * (E_t + 2) + 2 * y           # expf 2 u, the add 1 + e, the division
    safe = torch.ones_like(v, dtype=torch.bool)
    for s_, E_ in ((s1, E_s1), (s2, E_s2), (s3, E_s3)):
        safe &= (s_.abs() > 2 * U * E_).all(-1)
    return dict(y=y, E_y=E_y, inp=inp, h1=h1, E_h1=E_h1, h2=h2, E_h2=E_h2, h3=h3, E_h3=E_h3, s=s, E_s=E_s, safe=safe)


def crf_apply(v, feat, params, map_type, skip_learn=False):
    """crf_apply of kernels_loss.hip on INPUT values v (exact float32 numbers): (y, E_y, safe, extras)"""
    zero = torch.zeros_like(v)
    if map_type == "gamma":
        y = torch.pow(v, IG32)
        return y, 2 * POW_ULP * y.abs(), torch.ones_like(v, dtype=torch.bool), None
    if map_type == "learn" and not skip_learn:
        m = mlp(params, v, zero, feat)
        return m["y"], m["E_y"], m["safe"], m
    return v, zero, torch.ones_like(v, dtype=torch.bool), None


def luma_of(code, y, E_y):
    """y [..., 3] -> (luma [...], E): three products by a float32 constant (1.5 each) and two adds; avg: two adds and a division"""
    name = LUMA_CODE[code]
    if name == "avg":
        s = y.sum(-1)
        return s / 3, E_y.sum(-1) / 3 + y.abs().sum(-1)
    c = torch.tensor([float(np.float32(k)) for k in LUMA[name]], dtype=torch.float64, device=y.device)
    return (y * c).sum(-1), (E_y * c).sum(-1) + 3.5 * (y * c).abs().sum(-1)


def crf(x, feat, params, map_type, skip_learn=False, luma=-1):
    """evd_crf_forward: x [n, 3], feat None / [n, E] (shared by the three channels) / [n, 3, E]; returns (out, E, safe [n])"""
    x = _f64(x)
    dev = x.device
    ft = None
    if feat is not None:
        ft = _f64(feat, dev)
        ft = ft[:, None, :].expand(-1, 3, -1) if ft.ndim == 2 else ft
    p = unpack_params(params, dev) if params is not None else None
    y, E_y, safe, _ = crf_apply(x, ft, p, map_type, skip_learn)
    safe = safe.all(-1)
    if luma < 0:
        return y, E_y, safe
    l, E_l = luma_of(luma, y, E_y)
    return l[:, None], E_l[:, None], safe


# ---- event loss -----------------------------------------------------------------------------------------------------------------
def _event_common(start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, params, map_type, skip_learn, add_bii, tonemap_only, cmask, cw):
    dev = torch.as_tensor(start).device
    have0 = start0 is not None and end0 is not None
    src = [end, start] + ([end0, start0] if have0 else [])           # which: 0 end, 1 start, 2 end0, 3 start0
    x = torch.stack([_f64(t, dev) for t in src], 1)                 # [N, W, 3]
    N, Wn, _ = x.shape
    cn, cp = _f64(cum_neg, dev), _f64(cum_pos, dev)
    ch = torch.zeros(N, dtype=torch.long, device=dev)
    if cmask is not None:
        cm = torch.as_tensor(cmask).to(dev) != 0
        for k in range(3):
            ch = torch.where(cm[:, k], torch.full_like(ch, k), ch)   # the LAST set bit
    onehot = torch.nn.functional.one_hot(ch, 3).double()            # [N, 3]
    feat = None
    if add_bii == 1:
        feat = torch.stack([cn, cp], -1)[:, None, None, :].expand(N, Wn, 3, 2)
    elif add_bii == 2:
        feat = (torch.stack([cn, cp], -1)[:, None, :] * onehot[..., None])[:, None].expand(N, Wn, 3, 2)
    p = unpack_params(params, dev) if params is not None else None
    y, E_y, safe, m = crf_apply(x, feat, p, map_type, skip_learn)
    if tonemap_only:
        lum, E_lum = (y * onehot[:, None]).sum(-1), (E_y * onehot[:, None]).sum(-1)
        dlum_dy = onehot[:, None].expand(N, Wn, 3)
        E_coef = 0.0
    else:
        lum, E_lum = luma_of(0, y, E_y)
        c = torch.tensor([float(np.float32(k)) for k in LUMA["rec601"]], dtype=torch.float64, device=dev)
        dlum_dy = c.expand(N, Wn, 3)
        E_coef = 1.0
    eps = float(np.float32(1e-5))
    arg = lum + eps
    E_arg = E_lum + arg.abs()
    lg = torch.log(arg)
    E_lg = 2 * LOG_ULP * lg.abs() + E_arg / arg.abs()
    tn, tp = float(np.float32(thr_neg)), float(np.float32(thr_pos))
    bii = tn * cn + tp * cp
    E_bii = (tn * cn).abs() + (tp * cp).abs() + bii.abs()
    w = torch.ones(N, dtype=torch.float64, device=dev)
    if cmask is not None and cw is not None:
        w = torch.tensor([float(np.float32(k)) for k in cw], dtype=torch.float64, device=dev)[ch]
    pred = lg[:, 0::2] - lg[:, 1::2]                                 # [N, 1 or 2]: fine, coarse
    E_pred = E_lg[:, 0::2] + E_lg[:, 1::2] + pred.abs()
    d = pred - bii[:, None]
    E_d = E_pred + E_bii[:, None] + d.abs()
    nblocks = -(-N // 16)
    return dict(dev=dev, N=N, Wn=Wn, have0=have0, x=x, y=y, E_y=E_y, safe=safe.all(-1).all(-1), m=m, p=p, lum=lum, arg=arg, E_arg=E_arg, lg=lg,
                dlum_dy=dlum_dy, E_coef=E_coef, w=w, d=d, E_d=E_d, nblocks=nblocks, feat=feat)


def event_loss(start, end, cum_neg, cum_pos, thr_neg, thr_pos, start0=None, end0=None, params=None, map_type="none", skip_learn=False, add_bii=0,
               tonemap_only=False, cmask=None, cw=None):
    """partial[0..2] = sum w (pred - bii)^2 fine, the same coarse (0 without the pair), sum w; their bounds; `safe` [N]"""
    q = _event_common(start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, params, map_type, skip_learn, add_bii, tonemap_only, cmask, cw)
    t = q["d"] ** 2 * q["w"][:, None]
    E_t = 2 * q["d"].abs() * q["w"][:, None] * q["E_d"] + 2 * t.abs()
    n_red = 6 + 4 + q["nblocks"]                                     # 6 shuffles, 4 LDS adds, one atomic per block in any order
    part = torch.zeros(3, dtype=torch.float64, device=q["dev"])
    E = torch.zeros(3, dtype=torch.float64, device=q["dev"])
    part[0], E[0] = t[:, 0].sum(), E_t[:, 0].sum() + n_red * t[:, 0].abs().sum()
    if q["have0"]:
        part[1], E[1] = t[:, 1].sum(), E_t[:, 1].sum() + n_red * t[:, 1].abs().sum()
    part[2], E[2] = q["w"].sum(), n_red * q["w"].abs().sum() * (0.0 if bool((q["w"] == 1).all()) else 1.0)
    return dict(partial=part, E_partial=E, safe=q["safe"])


def event_loss_autograd(start, end, cum_neg, cum_pos, thr_neg, thr_pos, start0, end0, p, map_type, skip_learn, add_bii, tonemap_only, cmask, cw):
    """the two squared-error sums as plain torch ops on float64 leaves (p: dict of parameter tensors), for autograd"""
    N = start.shape[0]
    ch = torch.zeros(N, dtype=torch.long)
    if cmask is not None:
        for k in range(3):
            ch = torch.where(torch.as_tensor(cmask)[:, k] != 0, torch.full_like(ch, k), ch)
    onehot = torch.nn.functional.one_hot(ch, 3).double()
    f2 = torch.stack([cum_neg, cum_pos], -1)

    def enc(x):
        if map_type == "gamma":
            y = torch.pow(x, IG32)
        elif map_type == "learn" and not skip_learn:
            inp = torch.zeros(x.shape + (CRF_MAX_IN,), dtype=torch.float64)
            if add_bii == 1:
                inp[..., 1:3] = f2[:, None, :]
            elif add_bii == 2:
                inp[..., 1:3] = f2[:, None, :] * onehot[..., None]
            inp = torch.cat([x[..., None], inp[..., 1:]], -1)
            h = torch.relu(inp @ p["w0"].T + p["b0"])
            h = torch.relu(h @ p["w1"].T + p["b1"])
            h = torch.relu(h @ p["w2"].T + p["b2"])
            y = torch.sigmoid(0.1 * (h @ p["w3"] + p["b3"]) + x)
        else:
            y = x
        if tonemap_only:
            lum = (y * onehot).sum(-1)
        else:
            lum = (y * torch.tensor([float(np.float32(k)) for k in LUMA["rec601"]], dtype=torch.float64)).sum(-1)
        return torch.log(lum + float(np.float32(1e-5)))
    bii = float(np.float32(thr_neg)) * cum_neg + float(np.float32(thr_pos)) * cum_pos
    w = torch.ones(N, dtype=torch.float64)
    if cmask is not None and cw is not None:
        w = torch.tensor([float(np.float32(k)) for k in cw], dtype=torch.float64)[ch]
    fine = (((enc(end) - enc(start)) - bii) ** 2 * w).sum()
    coarse = (((enc(end0) - enc(start0)) - bii) ** 2 * w).sum() if start0 is not None else fine * 0
    return fine, coarse


def event_loss_bwd(start, end, cum_neg, cum_pos, thr_neg, thr_pos, g_fine, g_coarse, start0=None, end0=None, params=None, map_type="none",
                   skip_learn=False, add_bii=0, tonemap_only=False, cmask=None, cw=None):
    """hand-written backward of g_fine partial[0] + g_coarse partial[1]: d_start, d_end, d_start0, d_end0 [N, 3] and, for a live learn CRF,
    d_params [705] in the layout of evd_event_loss_bwd -- each with its bound"""
    q = _event_common(start, end, start0, end0, cum_neg, cum_pos, thr_neg, thr_pos, params, map_type, skip_learn, add_bii, tonemap_only, cmask, cw)
    dev, N, Wn = q["dev"], q["N"], q["Wn"]
    g = torch.tensor([g_fine, g_fine, g_coarse, g_coarse][:Wn], dtype=torch.float64, device=dev)
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0][:Wn], dtype=torch.float64, device=dev)
    rep = lambda t: t.repeat_interleave(2, dim=1)                     # per pair -> per which
    d, E_d = rep(q["d"]), rep(q["E_d"])
    w = q["w"][:, None]
    d_lg = sign * 2 * g * w * d
    E_d_lg = (2 * g * w).abs() * E_d + 3 * d_lg.abs()
    d_lum = d_lg / q["arg"]
    E_d_lum = E_d_lg / q["arg"].abs() + d_lum.abs() * (q["E_arg"] / q["arg"].abs() + 1)
    d_v = d_lum[..., None] * q["dlum_dy"]                             # [N, W, 3]
    E_d_v = E_d_lum[..., None] * q["dlum_dy"].abs() + 1.5 * q["E_coef"] * d_v.abs()
    out = {}
    x = q["x"]
    learn = map_type == "learn" and not skip_learn
    if map_type == "gamma":
        dg = IG32 * torch.pow(x, IG1_32)
        d_x = d_v * dg
        E_d_x = dg.abs() * E_d_v + d_x.abs() * (2 * POW_ULP + 2)
    elif learn:
        m, p = q["m"], q["p"]
        y, E_y = q["y"], q["E_y"]
        sg = y * (1 - y)
        E_sg = E_y * ((1 - y).abs() + y.abs()) + 2 * sg.abs()
        dz = d_v * sg
        E_dz = sg.abs() * E_d_v + d_v.abs() * E_sg + dz.abs()
        ds = 0.1 * dz
        E_ds = 0.1 * E_dz + 1.5 * ds.abs()
        m3, m2, m1 = (m["h3"] > 0).double(), (m["h2"] > 0).double(), (m["h1"] > 0).double()
        dh3 = m3 * ds[..., None] * p["w3"]
        E_dh3 = m3 * (p["w3"].abs() * E_ds[..., None] + dh3.abs())
        dh2 = m2 * (dh3 @ p["w2"])
        E_dh2 = m2 * (E_dh3 @ p["w2"].abs() + 16 * (dh3.abs() @ p["w2"].abs()))
        dh1 = m1 * (dh2 @ p["w1"])
        E_dh1 = m1 * (E_dh2 @ p["w1"].abs() + 16 * (dh2.abs() @ p["w1"].abs()))
        din0 = dh1 @ p["w0"][:, 0]
        E_din0 = E_dh1 @ p["w0"][:, 0].abs() + 16 * (dh1.abs() @ p["w0"][:, 0].abs())
        d_x = dz + din0
        E_d_x = E_dz + E_din0 + dz.abs() + din0.abs() + d_x.abs()
        # parameter gradient: per-lane contributions, wave_sum_dpp (4 DPP adds + 3), LDS atomics of the block's 4 wavefronts, one global
        # atomic per block -- all in arbitrary order
        n_p = 7 + 4 + q["nblocks"]

        def red(c, E_c):
            c, E_c = c.reshape((N * Wn * 3,) + c.shape[3:]), E_c.reshape((N * Wn * 3,) + c.shape[3:])
            return c.sum(0), E_c.sum(0) + n_p * c.abs().sum(0)

        def outer(a, E_a, b, E_b):
            c = a[..., :, None] * b[..., None, :]
            return red(c, E_a[..., :, None] * b.abs()[..., None, :] + a.abs()[..., :, None] * E_b[..., None, :] + c.abs())
        inp = m["inp"]
        gw0, E_gw0 = outer(dh1, E_dh1, inp, torch.zeros_like(inp))
        keep = torch.zeros(CRF_MAX_IN, dtype=torch.float64, device=dev)
        keep[:3] = 1                                                   # the kernel accumulates columns 0..2; the padding stays exactly 0
        gw0, E_gw0 = gw0 * keep, E_gw0 * keep
        gb0, E_gb0 = red(dh1, E_dh1)
        gw1, E_gw1 = outer(dh2, E_dh2, m["h1"], m["E_h1"])
        gb1, E_gb1 = red(dh2, E_dh2)
        gw2, E_gw2 = outer(dh3, E_dh3, m["h2"], m["E_h2"])
        gb2, E_gb2 = red(dh3, E_dh3)
        c3 = ds[..., None] * m["h3"]
        gw3, E_gw3 = red(c3, E_ds[..., None] * m["h3"].abs() + ds.abs()[..., None] * m["E_h3"] + c3.abs())
        gb3, E_gb3 = red(ds, E_ds)
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
        out["d_params"] = cat([gw0, gb0, gw1, gb1, gw2, gb2, gw3, gb3])
        out["E_d_params"] = cat([E_gw0, E_gb0, E_gw1, E_gb1, E_gw2, E_gb2, E_gw3, E_gb3])
    else:
        d_x, E_d_x = d_v, E_d_v
    names = ["d_end", "d_start", "d_end0", "d_start0"][:Wn]
    for k, nme in enumerate(names):
        out[nme], out["E_" + nme] = d_x[:, k], E_d_x[:, k]
    out["safe"] = q["safe"]
    return out
