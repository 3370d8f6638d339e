"""The kernels between the AWP embedding and the per-ray tail against the float64 reference of tests/awp_local_ref.py, on every dispatch arm:
evd_awp_feature_integration / _bwd (k_awp_integrate_c64, k_awp_integrate<1 | 2 | 4> and their backwards), evd_mam_local_forward
(k_mam_local_fwd_r<10, 8>, k_mam_local_fwd), evd_mam_local_backward (k_mam_local_bwd<false | true>) and evd_awp_local_consumers_backward
(k_local_consumers_bwd).  The entries are called through evdeblurnerf_amd._lib: the autograd nodes of awp.py hide `accumulate`, the absmax
word and the NULL arms.  Forward outputs are held to K = 2 times their first-order bound, backward outputs to the per-ray tolerances (scan
1e-5, MAM 2e-5, fused 2e-5); tests/test_awp_local_ref.py pins the reference, the inputs' conditions and what each structural mistake
would move.  Every test prints, per output, the worst ratio of error to bound or tolerance (<= 1 passes).

Worst ratios per arm (MI355X, measured on the commit that added this file, whose parent is df2cd4f; error / asserted bound for forward
outputs, per-ray error / tolerance for backward outputs; 1 would fail):
  scan  c64        out 0.14   d_feat 0.046  d_z 0.47   d_rays_d 0.019      (d_z: scan-c64-C64-N17-S9-zero_dir)
  scan  cpl1       out 0.14   d_feat 0.028  d_z 0.38   d_rays_d 0.021      (d_z: scan-cpl1-C20-N5-S33)
  scan  cpl2       out 0.14   d_feat 0.045  d_z 0.28   d_rays_d 0.012
  scan  cpl4       out 0.15   d_feat 0.083  d_z 0.32   d_rays_d 0.012      (d_z: scan-cpl4-C200-N5-S5)
  mam   fwd_r      alpha 0.026  beta 0.030  h_inter 0.055  h_intra 0.068  sum_alpha 0.0029  sum_beta 0.029  d_h 0.078  d_u 0.053
  mam   fwd        alpha 0.030  beta 0.032  h_inter 0.048  h_intra 0.058  sum_alpha 0.0030  sum_beta 0.015  d_h 0.058  d_u 0.057
  mam   flat       alpha - 1/S: 0.062 u / S (fwd_r), 0 (fwd);  beta - 1/P: 0.75 u / P (fwd_r), 0.5 u / P (fwd)
  fused consumers  d_h 0.027  d_u 0.036  d_z 0.032  d_rays_d 0.0081
No case failed and no kernel was changed: every NULL arm, accumulate = 0 / 1, the absmax word (its maximum, its NULL arm and the NaN ->
+inf promise) and the bit-for-bit equality of the fused kernel with the two-launch path at (2, 10, 129) and (1, 16, 512) hold as stated.
"""
import numpy as np
import pytest
import torch

import awp_local_ref as A

pytestmark = pytest.mark.gpu

SENT = 1234.5                                     # what an output holds before the call: an element the kernel skips stays visible
SCAN = [c["id"] for c in A.CASES if c["entry"] == "scan"]
MAM = [c["id"] for c in A.CASES if c["entry"] == "mam"]
FUSED = [c["id"] for c in A.CASES if c["entry"] == "fused"]


def L():
    from evdeblurnerf_amd import _lib
    return _lib


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def full(shape, value=SENT, dtype=torch.float32):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def report(cid, **ratios):
    print(f"[awp-local] {cid}: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1}
    assert not bad, (cid, bad)


# ---- the scan -----------------------------------------------------------------------------------------------------------------------
def scan_fwd(feat, z, rd):
    l = L()
    N, S, C = feat.shape
    out = full((max(N, 1), C))
    a = [T(t) for t in (feat, z, rd)]                    # kept alive until the kernel has run
    l.check(l.lib().evd_awp_feature_integration(l.ptr(a[0]), l.ptr(a[1]), l.ptr(a[2]), N, S, C, l.ptr(out), l.stream_ptr()), "evd_awp_feature_integration")
    return host(out)[0]


def scan_bwd(feat, z, rd, g, want_z=True, want_d=True):
    l = L()
    N, S, C = feat.shape
    d_feat, d_z, d_rd = full((max(N, 1), S, C)), full((max(N, 1), S)) if want_z else None, full((max(N, 1), 3)) if want_d else None
    a = [T(t) for t in (feat, z, rd, g)]
    l.check(l.lib().evd_awp_feature_integration_bwd(l.ptr(a[0]), l.ptr(a[1]), l.ptr(a[2]), l.ptr(a[3]), N, S, C, l.ptr(d_feat), l.ptr(d_z), l.ptr(d_rd),
                                                    l.stream_ptr()), "evd_awp_feature_integration_bwd")
    return host(d_feat, d_z, d_rd)


@pytest.mark.parametrize("cid", SCAN)
def test_scan(cid):
    """forward within its bound on every ray; backward per ray within 1e-5 on the unsaturated rays (exactly 0 where the float64
    gradient is: a zero direction, S = 1) and finite on the saturated one; null_arms: d_z = NULL, d_rays_d = NULL and both leave the
    bits of every output that is still written"""
    case = A.BY_ID[cid]
    x, r = A.reference(cid)
    N, tol = case["N"], A.TOL["scan"]
    ok = np.ones(N, bool)
    ok[x["sat"]] = False
    out = scan_fwd(x["feat"], x["z"], x["rays_d"])
    d_feat, d_z, d_rd = scan_bwd(x["feat"], x["z"], x["rays_d"], x["g"])
    for name, t in (("d_feat", d_feat), ("d_z", d_z), ("d_rays_d", d_rd)):
        assert np.isfinite(t).all(), name                                             # the float64 backward is finite on every ray (CPU test)
    report(cid, out=A.bound_ratio(out, r["out"], r["E_out"]),
           d_feat=A.per_ray_rel(d_feat, r["d_feat"], N)[ok].max() / tol, d_z=A.per_ray_rel(d_z, r["d_z"], N)[ok].max() / tol,
           d_rays_d=A.rays_d_rel(d_rd, r["d_rays_d"], r["E_d_rays_d"], tol)[ok].max() / tol)
    if case["variant"] == "null_arms":
        for want_z, want_d in ((False, True), (True, False), (False, False)):
            f2, z2, d2 = scan_bwd(x["feat"], x["z"], x["rays_d"], x["g"], want_z, want_d)
            assert same_bits(f2, d_feat), (want_z, want_d)
            assert not want_z or same_bits(z2, d_z)
            assert not want_d or same_bits(d2, d_rd)


@pytest.mark.parametrize("C", [64, 20, 127, 200])
def test_scan_without_rays_writes_nothing(C):
    rs = np.random.RandomState(C)
    feat, z, rd, g = (rs.uniform(0.1, 1, s).astype(np.float32) for s in ((0, 3, C), (0, 3), (0, 3), (0, C)))
    pad = lambda a: np.zeros((1,) + a.shape[1:], np.float32)                           # the entries want non-null pointers
    l = L()
    out, d_feat, d_z, d_rd = full((1, C)), full((1, 3, C)), full((1, 3)), full((1, 3))
    a = [T(pad(t)) for t in (feat, z, rd, g)]
    l.check(l.lib().evd_awp_feature_integration(l.ptr(a[0]), l.ptr(a[1]), l.ptr(a[2]), 0, 3, C, l.ptr(out), l.stream_ptr()), "evd_awp_feature_integration")
    l.check(l.lib().evd_awp_feature_integration_bwd(l.ptr(a[0]), l.ptr(a[1]), l.ptr(a[2]), l.ptr(a[3]), 0, 3, C, l.ptr(d_feat), l.ptr(d_z), l.ptr(d_rd),
                                                    l.stream_ptr()), "evd_awp_feature_integration_bwd")
    for t in host(out, d_feat, d_z, d_rd):
        assert (t == SENT).all()


@pytest.mark.parametrize("S,C", [(4, 257), (0, 64), (0, 20)])
def test_scan_rejects_257_channels_and_no_samples(S, C):
    """host-side argument checks: they return before any launch"""
    feat, z, rd, g = (T(np.ones(s, np.float32)) for s in ((2, max(S, 1), C), (2, max(S, 1)), (2, 3), (2, C)))
    l = L()
    out, d_feat = full((2, C)), full((2, max(S, 1), C))
    with pytest.raises(l.EvdError):
        l.check(l.lib().evd_awp_feature_integration(l.ptr(feat), l.ptr(z), l.ptr(rd), 2, S, C, l.ptr(out), l.stream_ptr()))
    with pytest.raises(l.EvdError):
        l.check(l.lib().evd_awp_feature_integration_bwd(l.ptr(feat), l.ptr(z), l.ptr(rd), l.ptr(g), 2, S, C, l.ptr(d_feat), None, None, l.stream_ptr()))
    assert (host(out)[0] == SENT).all() and (host(d_feat)[0] == SENT).all()


# ---- the MAM's per-sample part ------------------------------------------------------------------------------------------------------
def mam_fwd(h, u, R, P, S, C=A.MAM_C):
    """the kernel's own forward: device tensors h_inter, h_intra, alpha, beta (sentinel-filled before the call)"""
    l = L()
    o = full((max(R, 1), P, 64)), full((max(R, 1), S, 64)), full((max(R, 1), P, S)), full((max(R, 1), P, S))
    l.check(l.lib().evd_mam_local_forward(l.ptr(h), l.ptr(u), R, P, S, C, l.ptr(o[0]), l.ptr(o[1]), l.ptr(o[2]), l.ptr(o[3]), l.stream_ptr()), "evd_mam_local_forward")
    return o


def mam_bwd(h, u, fwd, g_inter, g_intra, R, P, S, accumulate=0, prefill=None, absmax=True, C=A.MAM_C):
    """(d_h_local, d_u_partial, absmax word) as numpy; d_h_local starts as the sentinel (or the prefill), the word as 7"""
    l = L()
    d_h = full(h.shape) if prefill is None else (prefill if isinstance(prefill, torch.Tensor) else T(prefill)).clone()
    d_u, word = full((max(R, 1), 64)), full((1,), 7, torch.int32) if absmax else None
    l.check(l.lib().evd_mam_local_backward(l.ptr(h), l.ptr(u), l.ptr(fwd[2]), l.ptr(fwd[3]), l.ptr(fwd[0]), l.ptr(fwd[1]), l.ptr(g_inter), l.ptr(g_intra), R, P, S, C,
                                           l.ptr(d_h), l.ptr(d_u), accumulate, l.ptr(word), l.stream_ptr()), "evd_mam_local_backward")
    return host(d_h, d_u, word)


def absmax_bits(d_h):
    return int(np.abs(d_h).max().astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("cid", MAM)
def test_mam(cid):
    """forward: alpha, beta, h_inter, h_intra within their bounds, alpha's rows and beta's columns summing to 1 within theirs (flat: 1 / S
    and 1 / P to the rounding of the division).  Backward on the kernel's own forward: d h_local per sub-exposure ray and d u per ray
    within 2e-5 with accumulate = 0 into a sentinel-filled tensor; accumulate = 1 = prefill + that result to one rounding; the absmax
    word (started at 7) is the bit pattern of max |d h_local| of the kernel's own output, NULL leaves the other bits, and one NaN in
    ray 0's d_inter makes it +inf and leaves every other ray's bits"""
    case = A.BY_ID[cid]
    x, r = A.reference(cid)
    R, P, S, tol = case["R"], case["P"], case["S"], A.TOL["mam"]
    h, u, gi, gs = T(x["h"]), T(x["u"]), T(x["g_inter"]), T(x["g_intra"])
    fwd = mam_fwd(h, u, R, P, S)
    h_inter, h_intra, alpha, beta = host(*fwd)
    ratios = {k: A.bound_ratio(v, r[k], r["E_" + k]) for k, v in (("alpha", alpha), ("beta", beta), ("h_inter", h_inter), ("h_intra", h_intra))}
    ratios["sum_alpha"] = A.bound_ratio(alpha.astype(np.float64).sum(-1), np.ones((R, P)), r["E_alpha"].sum(-1))
    ratios["sum_beta"] = A.bound_ratio(beta.astype(np.float64).sum(-2), np.ones((R, S)), r["E_beta"].sum(-2))
    if case["variant"] == "flat":
        ratios["flat_alpha"] = float(np.abs(alpha.astype(np.float64) - 1 / S).max() / (A.U / S))
        ratios["flat_beta"] = float(np.abs(beta.astype(np.float64) - 1 / P).max() / (A.U / P))
    d_h, d_u, word = mam_bwd(h, u, fwd, gi, gs, R, P, S)
    ratios["d_h"] = A.per_ray_rel(d_h, r["d_h"], R * P).max() / tol
    ratios["d_u"] = A.per_ray_rel(d_u, r["d_u"], R).max() / tol
    report(cid, **ratios)
    assert int(word.view(np.uint32)[0]) == absmax_bits(d_h)
    d_h2, d_u2, _ = mam_bwd(h, u, fwd, gi, gs, R, P, S, absmax=False)
    assert same_bits(d_h2, d_h) and same_bits(d_u2, d_u)
    d_h1, d_u1, word1 = mam_bwd(h, u, fwd, gi, gs, R, P, S, accumulate=1, prefill=x["prefill"])
    want = x["prefill"].astype(np.float64) + d_h.astype(np.float64)
    assert (np.abs(d_h1 - want) <= A.U * np.abs(want)).all()
    assert same_bits(d_u1, d_u) and int(word1.view(np.uint32)[0]) == absmax_bits(d_h1)
    if case["variant"] is None:
        gn = x["g_inter"].copy()
        gn[0, 0, 0] = np.nan
        d_hn, _, wordn = mam_bwd(h, u, fwd, T(gn), gs, R, P, S)
        assert int(wordn.view(np.uint32)[0]) == 0x7f800000
        assert same_bits(d_hn[P:], d_h[P:])


def test_mam_without_rays_writes_nothing():
    P, S = 3, 5
    h, u = full((P, S, 64), 0.5), full((64,), 0.1)
    fwd = mam_fwd(h, u, 0, P, S)
    for t in host(*fwd):
        assert (t == SENT).all()
    d_h, d_u, word = mam_bwd(h, u, fwd, full((1, P, 64), 1.0), full((1, S, 64), 1.0), 0, P, S)
    assert (d_h == SENT).all() and (d_u == SENT).all() and int(word[0]) == 7
    out = fused_bwd(h, u, fwd, full((1, P, 64), 1.0), full((1, S, 64), 1.0), full((P, S), 0.5), full((P, 3), 1.0), full((P, 64), 1.0), 0, P, S)
    assert all((t == SENT).all() for t in out[:4]) and int(out[4][0]) == 7


@pytest.mark.parametrize("P,S,C", [(17, 8, 64), (4, 513, 64), (4, 8, 32)])
def test_mam_entries_reject_what_they_are_not_built_for(P, S, C):
    """host-side argument checks of the three entries: they return before any launch"""
    l = L()
    h, u = full((P, S, 64), 0.5), full((64,), 0.1)
    with pytest.raises(l.EvdError):
        mam_fwd(h, u, 1, P, S, C)
    fwd = full((1, P, 64)), full((1, S, 64)), full((1, P, S)), full((1, P, S))
    with pytest.raises(l.EvdError):
        mam_bwd(h, u, fwd, full((1, P, 64)), full((1, S, 64)), 1, P, S, C=C)
    with pytest.raises(l.EvdError):
        fused_bwd(h, u, fwd, full((1, P, 64)), full((1, S, 64)), full((P, S)), full((P, 3)), full((P, 64)), 1, P, S, C=C)


# ---- the fused backward of h_local's two consumers ------------------------------------------------------------------------------------
def fused_bwd(h, u, fwd, g_inter, g_intra, z, rd, g_int, R, P, S, want_z=True, want_d=True, absmax=True, C=A.MAM_C):
    """(d_h_local, d_u_partial, d_z, d_rays_d, absmax word) as numpy, every output sentinel-filled before the call"""
    l = L()
    d_h, d_u = full(h.shape), full((max(R, 1), 64))
    d_z, d_rd, word = full(z.shape) if want_z else None, full(rd.shape) if want_d else None, full((1,), 7, torch.int32) if absmax else None
    l.check(l.lib().evd_awp_local_consumers_backward(l.ptr(h), l.ptr(u), l.ptr(fwd[2]), l.ptr(fwd[3]), l.ptr(fwd[0]), l.ptr(fwd[1]), l.ptr(g_inter), l.ptr(g_intra),
                                                     l.ptr(z), l.ptr(rd), l.ptr(g_int), R, P, S, C, l.ptr(d_h), l.ptr(d_u), l.ptr(d_z), l.ptr(d_rd), l.ptr(word),
                                                     l.stream_ptr()), "evd_awp_local_consumers_backward")
    return host(d_h, d_u, d_z, d_rd, word)


@pytest.mark.parametrize("cid", FUSED)
def test_fused_consumers_backward(cid):
    """k_local_consumers_bwd against the float64 sum of the two shares (not against the kernels it fuses): d h_local, d z per
    sub-exposure ray, d u per ray within 2e-5, d rays_d against its floor; sub-exposure ray 1 has a zero direction (exact zeros), ray 2
    a repeated z.  The NULL arms of d_z, d_rays_d and the absmax word leave the other bits; the word is max |d h_local|; d h_local,
    d u_partial and the word have the bits of the two-launch path (the scan's backward, then the MAM's with accumulate = 1)"""
    case = A.BY_ID[cid]
    x, r = A.reference(cid)
    R, P, S, tol = case["R"], case["P"], case["S"], A.TOL["fused"]
    h, u, gi, gs, z, rd, g = (T(x[k]) for k in ("h", "u", "g_inter", "g_intra", "z", "rays_d", "g_int"))
    fwd = mam_fwd(h, u, R, P, S)
    d_h, d_u, d_z, d_rd, word = fused_bwd(h, u, fwd, gi, gs, z, rd, g, R, P, S)
    for name, t in (("d_h", d_h), ("d_u", d_u), ("d_z", d_z), ("d_rays_d", d_rd)):
        assert np.isfinite(t).all(), name
    report(cid, d_h=A.per_ray_rel(d_h, r["d_h"], R * P).max() / tol, d_u=A.per_ray_rel(d_u, r["d_u"], R).max() / tol,
           d_z=A.per_ray_rel(d_z, r["d_z"], R * P).max() / tol, d_rays_d=A.rays_d_rel(d_rd, r["d_rays_d"], r["E_d_rays_d"], tol).max() / tol)
    assert int(word.view(np.uint32)[0]) == absmax_bits(d_h)
    for want_z, want_d, absmax in ((False, True, True), (True, False, True), (False, False, True), (True, True, False)):
        o = fused_bwd(h, u, fwd, gi, gs, z, rd, g, R, P, S, want_z, want_d, absmax)
        assert same_bits(o[0], d_h) and same_bits(o[1], d_u), (want_z, want_d, absmax)
        assert not want_z or same_bits(o[2], d_z)
        assert not want_d or same_bits(o[3], d_rd)
        assert not absmax or same_bits(o[4], word)
    l = L()
    d_h2 = full(h.shape)
    l.check(l.lib().evd_awp_feature_integration_bwd(l.ptr(h), l.ptr(z), l.ptr(rd), l.ptr(g), R * P, S, 64, l.ptr(d_h2), None, None, l.stream_ptr()),
            "evd_awp_feature_integration_bwd")
    d_h2, d_u2, word2 = mam_bwd(h, u, fwd, gi, gs, R, P, S, accumulate=1, prefill=d_h2)
    assert same_bits(d_h2, d_h) and same_bits(d_u2, d_u) and same_bits(word2, word)
