"""Pins tests/awp_local_ref.py -- the float64 reference, the bounds and the case matrix that tests/test_gpu_awp_local.py holds the AWP scan
and MAM per-sample kernels to -- before any kernel sees it: to the goldens the real reference computed (G15, G22), the reduced MAM formula
to the unreduced module in float64 (values and gradients), the matrix to the dispatch it claims to cover, the stated input conditions
(unsaturated / saturated rays, peaked and flat softmaxes, the exact zeros), a float32 torch evaluation of every case to a tenth of each
tolerance and to every forward bound at factor 1, and every entry of FAULTS to a visible move on every arm it can reach.  CPU only."""
import numpy as np
import pytest
import torch

import awp_local_ref as A
from conftest import load_golden

IDS = [c["id"] for c in A.CASES]


def _rel(a, b, floor=1e-300):
    """largest difference relative to the largest reference value (or to `floor`: the unit scale of the data, where the reference is 0)"""
    a, b = A._np64(a), A._np64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def test_integrate64_reproduces_G15():
    """the golden is the reference's float32 torch result: held to the forward bound like a kernel"""
    g = load_golden("G15_awp_feature_integration")
    for tag in ("a", "b"):
        feat = g[f"{tag}_feat"]
        S, C = feat.shape[-2:]
        r = A.integrate64(feat.reshape(-1, S, C), g[f"{tag}_z"], g[f"{tag}_rays_d"])
        assert A.bound_ratio(g[f"{tag}_out"].reshape(-1, C), r["out"], r["E_out"]) <= 1, tag


def test_mam_local64_reproduces_G22():
    """the reduced sums pushed through the golden's own linear against the tensors the real module handed on: float32 resolution"""
    g = load_golden("G22_mam")
    R, P = g["x_global"].shape[:2]
    S = g["x_local"].shape[1]
    Wl, bl, v = (g[k].astype(np.float64) for k in ("sd.linear.weight", "sd.linear.bias", "sd.Corr.line_conv_att.weight"))
    r = A.mam_local64(g["x_local"], Wl.T @ v.reshape(-1), R, P, S)
    for name, hsum in (("inter", r["h_inter"]), ("intra", r["h_intra"])):
        got = (hsum.numpy() @ Wl.T + bl).transpose(0, 2, 1)
        assert np.abs(got - g[name]).max() <= 8 * A.U * max(1.0, np.abs(g[name]).max()), name


@pytest.mark.parametrize("R,P,S", [(2, 3, 5), (1, 16, 40), (3, 1, 1)])
def test_reduced_mam_equals_the_unreduced_module(R, P, S):
    """u = W^T v: values of both sums and the gradients w.r.t. h_local and line_conv_att.weight (d v = W d u) to 1e-12, against autograd
    of linear / 1x1 conv / two softmaxes / two sums;  the hand-written backward also against autograd of the reduced formula"""
    rs = np.random.RandomState(R * 100 + S)
    h = np.maximum(rs.standard_normal((R * P, S, 64)), 0)
    Wl, bl, v = rs.standard_normal((32, 64)) * 0.125, rs.standard_normal(32) * 0.1, rs.standard_normal(32) * 0.5
    Gi, Gs = rs.standard_normal((R, 32, P)), rs.standard_normal((R, 32, S))
    full = A.mam_unreduced64(h, Wl, bl, v, R, P, S, Gi, Gs)
    gi, gs = Gi.transpose(0, 2, 1) @ Wl, Gs.transpose(0, 2, 1) @ Wl                    # the caller's 64 -> 32 map, backward
    u = Wl.T @ v
    r = A.mam_local64(h, u, R, P, S, gi, gs)
    assert _rel((r["h_inter"].numpy() @ Wl.T + bl).transpose(0, 2, 1), full["inter"]) < 1e-12
    assert _rel((r["h_intra"].numpy() @ Wl.T + bl).transpose(0, 2, 1), full["intra"]) < 1e-12
    assert _rel(r["d_h"], full["d_h"]) < 1e-12
    assert _rel(Wl @ r["d_u"].sum(0).numpy(), full["d_v"], floor=1.0) < 1e-12          # P = S = 1: d v is 0
    auto = A.mam_local64_autograd(h, u, R, P, S, gi, gs)
    for k in ("alpha", "beta", "h_inter", "h_intra", "d_h", "d_u"):
        assert _rel(r[k], auto[k], floor=1.0) < 1e-12, k


def test_case_matrix_names_every_arm():
    for c in A.CASES:
        assert A.expected_arm(c) == c["arm"], c["id"]
    have = {(c["entry"], c["arm"]) for c in A.CASES}
    assert have == {(e, a) for e, arms in A.ARMS.items() for a in arms}
    scan = {(c["C"], c["N"], c["S"]) for c in A.CASES if c["entry"] == "scan" and c["variant"] is None}
    assert {(64, N, 5) for N in (1, 15, 16, 17, 33)} | {(64, 17, S) for S in (1, 2, 3, 4, 5, 9, 128)} <= scan
    for Cs, Ss in (((1, 20, 63), (1, 2, 5, 8, 9, 33)), ((65, 127, 128), (1, 2, 3, 4, 5, 33)), ((129, 200, 256), (1, 2, 3, 4, 5, 33))):
        assert {C for C, _, _ in scan} >= set(Cs)
        assert {(Cs[1], N, 5) for N in (1, 3, 4, 5)} | {(Cs[1], 5, S) for S in Ss} <= scan
    for arm in A.ARMS["scan"]:
        assert {c["variant"] for c in A.CASES if c["arm"] == arm} >= {"zero_dir", "repeat_z", "null_arms", "saturated"}
    mam = {(c["arm"], c["R"], c["P"], c["S"], c["variant"]) for c in A.CASES if c["entry"] == "mam"}
    assert {("fwd_r", *s, None) for s in ((1, 1, 1), (2, 1, 33), (2, 7, 16), (2, 7, 17), (2, 10, 127), (3, 10, 128))} <= mam
    assert {("fwd", *s, None) for s in ((2, 11, 128), (2, 10, 129), (2, 16, 1), (2, 3, 300), (1, 16, 512))} <= mam
    assert {(arm, *s, v) for arm, s in (("fwd_r", (2, 7, 17)), ("fwd", (2, 11, 128))) for v in ("peaked", "flat")} <= mam
    fused = {(c["R"], c["P"], c["S"]) for c in A.CASES if c["entry"] == "fused"}
    assert fused == {(2, 3, 1), (2, 3, 2), (3, 10, 33), (2, 10, 129), (1, 16, 18), (1, 16, 512)}
    assert len([c for c in A.CASES if c["entry"] == "scan"]) >= 40


def _scan_conditions(feat, z, d, sat_rays, grads, case):
    """the stated conditions of a scan-shaped problem (also the integration half of a fused case); grads: the float64 d feat, d z, d rays_d"""
    N, S = z.shape
    fd = A.max_fd(feat, z, d)
    sat = np.zeros(N, bool)
    sat[sat_rays] = True
    assert (fd[~sat] <= A.FD_CAP).all() and (fd[sat] >= A.FD_SAT).all(), fd
    assert (fd[~sat & (fd > 0)] >= A.FD_FLOOR).all(), fd
    assert case["variant"] != "saturated" or sat.any()
    zero = np.flatnonzero((d == 0).all(1)) if S > 1 else np.arange(N)                 # a zero direction, or S = 1: no interval at all
    assert case["variant"] != "zero_dir" or 0 in zero
    for k, t in grads.items():
        assert np.isfinite(A._np64(t)).all() and (A._np64(t)[zero] == 0).all(), k
    if case["variant"] == "repeat_z" or case["entry"] == "fused" and S >= 3:
        assert (np.diff(z, axis=-1) == 0).any()


@pytest.mark.parametrize("cid", IDS)
def test_conditions_and_float32_evaluation(cid):
    """every case: the input conditions hold, and torch float32 of the same formulas lies within each forward bound at factor 1 (K = 2 is
    asserted of the kernels) and within a tenth of each backward tolerance"""
    case = A.BY_ID[cid]
    x, r = A.reference(cid)
    m = A.float32_margins(case, x, r)
    want = {"scan": {"out", "d_feat", "d_z", "d_rays_d"}, "mam": {"alpha", "beta", "h_inter", "h_intra", "d_h", "d_u"}, "fused": {"d_h", "d_u", "d_z", "d_rays_d"}}
    assert set(m) == want[case["entry"]] and max(m.values()) <= 1, m
    if case["entry"] == "scan":
        assert np.isfinite(r["out"].numpy()).all()
        _scan_conditions(x["feat"], x["z"], x["rays_d"], x["sat"], {k: r[k] for k in ("d_feat", "d_z", "d_rays_d")}, case)
        return
    R, P, S = case["R"], case["P"], case["S"]
    if case["entry"] == "mam":
        a = (A._t64(x["h"]).reshape(R, P, S, 64) @ A._t64(x["u"])).numpy()
        if case["variant"] == "peaked":
            assert np.ptp(a, axis=-1).max() >= A.SPREAD
        if case["variant"] == "flat":
            assert (r["alpha"].numpy() == 1 / S).all() and (r["beta"].numpy() == 1 / P).all()
            h4 = x["h"].astype(np.float64).reshape(R, P, S, 64)
            assert _rel(r["h_inter"], h4.mean(2)) < 1e-14 and _rel(r["h_intra"], h4.mean(1)) < 1e-14
        return
    _scan_conditions(x["h"], x["z"], x["rays_d"], [], dict(d_feat=r["d_h_scan"], d_z=r["d_z"], d_rays_d=r["d_rays_d"]), case)


def moves(case, fault):
    """whether the mistake moves an output the GPU test compares on this case: a forward output by more than 4 x the asserted bound, a
    backward output (per ray) by more than 10 x its tolerance"""
    x, r = A.reference(case["id"])
    _, bad = A.reference(case["id"], fault)
    tol, e = A.TOL[case["entry"]], case["entry"]
    if e == "scan":
        N = case["N"]
        sat = np.zeros(N, bool)
        sat[x["sat"]] = True
        if fault == "missing_1e-10":          # the saturated ray's backward: the kernels' divisor is 0 there without the term (held to finiteness)
            return bool((A.per_ray_rel(bad["d_feat"], r["d_feat"], N)[sat] > 10 * tol).any())
        if A.bound_ratio(bad["out"], r["out"], r["E_out"]) > 4:
            return True
        rel = np.maximum(A.per_ray_rel(bad["d_feat"], r["d_feat"], N), A.per_ray_rel(bad["d_z"], r["d_z"], N))
        rel = np.maximum(rel, A.rays_d_rel(bad["d_rays_d"], r["d_rays_d"], r["E_d_rays_d"], tol))
        return bool((rel[~sat] > 10 * tol).any())
    R, P = case["R"], case["P"]
    if e == "mam" and any(A.bound_ratio(bad[k], r[k], r["E_" + k]) > 4 for k in ("alpha", "beta", "h_inter", "h_intra")):
        return True
    if A.per_ray_rel(bad["d_h"], r["d_h"], R * P).max() > 10 * tol or A.per_ray_rel(bad["d_u"], r["d_u"], R).max() > 10 * tol:
        return True
    return e == "fused" and (A.per_ray_rel(bad["d_z"], r["d_z"], R * P).max() > 10 * tol
                             or A.rays_d_rel(bad["d_rays_d"], r["d_rays_d"], r["E_d_rays_d"], tol).max() > 10 * tol)


@pytest.mark.parametrize("fault", list(A.FAULTS))
def test_every_fault_shows_on_every_arm_it_reaches(fault):
    reached = {}
    for c in sorted(A.CASES, key=lambda c: c["S"] * c.get("C", 64) * c.get("N", c.get("R", 1) * c.get("P", 1))):
        key = (c["entry"], c["arm"])
        if A.fault_reaches(fault, c) and not reached.get(key):
            reached[key] = moves(c, fault)
    assert reached and all(reached.values()), (fault, reached)
