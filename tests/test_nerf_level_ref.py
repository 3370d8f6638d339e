"""CPU tests of tests/nerf_level_ref.py, the float64 reference, mode model, bounds and case matrix of
tests/test_gpu_nerf_level_forward.py: the use_viewdirs=False head and the two feature outputs against the oracle (the view-branch raw is
pinned by golden G40, tests/test_nerf_generic_ref.py), the case matrix against the dispatch it restates, and -- without running a kernel --
that every bound stays below what each structural fault of the restatement changes, by 10 x in the float32-grade modes, 2 x in f16 and
more than 1 x in bf16.  The module prints the worst (smallest) ratio per mode at its end.

The 1 x 1 cases are not swept: one sample under-reads every fault (a unit fault needs a sample on which the unit is live), and each
network of a 1 x 1 case is swept at its other sizes.  Nor is the (CUs + 1) x 128 case of f16c, whose size is the device's; its network
is swept at four other sizes and its bound is the float32-grade floor alone."""
import functools

import numpy as np
import pytest

import nerf_level_ref as V
from evdeblurnerf_amd import weights as W

WORST = {}
GEOMS = sorted({(c["net"], c["rgb_bias"], c["R"], c["S"]) for c in V.CASES if c["R"] is not None and c["R"] * c["S"] > 1})
OUTS = ("raw", "feature1", "feature2")


@functools.lru_cache(maxsize=None)
def sweep(net, rgb_bias, R, S):
    """(exact outputs, {mode: quantised outputs}, {fault: ({output: L-inf change}, unit picked)}) of a network on inputs(R, S), once"""
    ex = V.evaluate_net(net, R, S, rgb_bias)
    qm = {m: V.evaluate_net(net, R, S, rgb_bias, quant=m) for m in V.QUANT}
    changes = {}
    for f in V.faults_of(net, rgb_bias, kind=2):
        bad = V.evaluate_net(net, R, S, rgb_bias, fault=f)
        changes[f] = ({k: float((bad[k] - ex[k]).abs().max()) for k in OUTS if ex[k] is not None}, bad.get("unit"))
    return ex, qm, changes


def ratio(c, fault):
    """the change a fault makes to an output the case compares, over that output's bound: the largest over the case's outputs"""
    ex, qm, changes = sweep(c["net"], c["rgb_bias"], c["R"], c["S"])
    best = 0.0
    for k in ("raw",) + ((f"feature{c['kind']}",) if c["kind"] else ()):
        bound, _ = V.bound_of(ex[k], qm[c["mode"]][k] if c["mode"] in qm else None, ex["A"])
        best = max(best, changes[fault][0][k] / bound)
    return best


def swept(c):
    return (c["net"], c["rgb_bias"], c["R"], c["S"]) in GEOMS


def blind_key(c, fault):
    return (c["net"], c["R"], c["S"], c["kind"], fault)


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\n  mode    pairs  worst ratio (change / bound)  case, fault")
    for m, (n, r, what) in sorted(WORST.items()):
        print(f"  {m:6s} {n:6d}  {r:11.2f}                   {what}")


@pytest.mark.parametrize("net,rgb_bias,R,S", GEOMS, ids=[f"{g[0]}-{g[2]}x{g[3]}" + ("" if g[1] else "-norgbbias") for g in GEOMS])
def test_every_fault_is_live_and_exceeds_the_bounds(net, rgb_bias, R, S):
    """No fault is dead: each changes the restatement, and a unit fault found a live unit.  For every case on these inputs and every fault
    that applies to it, the change is at least VISIBLE[mode] bounds (bf16: more than one, or the pair is listed in BF16_BLIND -- and a
    listed pair is blind indeed, so the list cannot go stale)."""
    ex, qm, changes = sweep(net, rgb_bias, R, S)
    assert ex["A"] < 8.0
    for f, (ch, unit) in changes.items():
        assert max(ch.values()) > 0, f
        if f.startswith(("hid", "swap", "last_hv")):
            assert unit is not None, f
    for c in V.CASES:
        if (c["net"], c["rgb_bias"], c["R"], c["S"]) != (net, rgb_bias, R, S):
            continue
        for f in V.faults_of(net, rgb_bias, c["kind"]):
            r = ratio(c, f)
            n, w, what = WORST.get(c["mode"], (0, float("inf"), ""))
            WORST[c["mode"]] = (n + 1,) + ((r, f"{c['id']}, {f}") if r < w else (w, what))
            if c["mode"] == "bf16":
                assert (r > 1.0) != (blind_key(c, f) in V.BF16_BLIND), (c["id"], f, r)
            else:
                assert r >= V.VISIBLE[c["mode"]], (c["id"], f, r)


def test_bf16_blind_is_a_small_list_and_every_arm_still_sees_every_fault():
    bf16 = [c for c in V.CASES if c["mode"] == "bf16" and swept(c)]
    pairs = [(c, f) for c in bf16 for f in V.faults_of(c["net"], c["rgb_bias"], c["kind"])]
    assert len(set(V.BF16_BLIND)) == len(V.BF16_BLIND) and set(V.BF16_BLIND) <= {blind_key(c, f) for c, f in pairs}
    print(f"BF16_BLIND holds {len(V.BF16_BLIND)} of {len(pairs)} bf16 (case, fault) pairs")
    assert 10 * len(V.BF16_BLIND) <= len(pairs)
    for arm in sorted({c["arm"] for c in bf16}):
        faults = {f for c, f in pairs if c["arm"] == arm}
        seen = {f for c, f in pairs if c["arm"] == arm and ratio(c, f) > 1.0}
        assert seen == faults, (arm, sorted(faults - seen))


def test_half_precision_bounds_are_small_against_raw():
    """a case's f16 bound on raw is below 1 % of max |raw|, its bf16 bound below 5 %"""
    worst = {"f16": 0.0, "bf16": 0.0}
    for c in V.CASES:
        if c["mode"] in V.QUANT and swept(c):
            ex, qm, _ = sweep(c["net"], c["rgb_bias"], c["R"], c["S"])
            bound, _ = V.bound_of(ex["raw"], qm[c["mode"]]["raw"], ex["A"])
            share = bound / float(ex["raw"].abs().max())
            worst[c["mode"]] = max(worst[c["mode"]], share)
            assert share < {"f16": 0.01, "bf16": 0.05}[c["mode"]], (c["id"], share)
    print(f"largest bound on raw / max |raw|: f16 {worst['f16']:.4f}, bf16 {worst['bf16']:.4f}")


def test_case_ids_are_unique_and_name_the_arm_their_construction_reaches():
    ids = [c["id"] for c in V.CASES]
    assert len(set(ids)) == len(ids)
    for c in V.CASES:
        assert V.expected_arm(c) == c["arm"], c["id"]
        assert (c["R"], c["S"]) in V.SIZES or (c["R"] is None and c["S"] == 128 and c["mode"] == "f16c"), c["id"]
    modes = {}
    for c in V.CASES:
        modes.setdefault(c["arm"], set()).add(c["mode"])
    assert modes == {"c": {"f16c"}, "pipe": set(V.HALF), "pipe_feat": set(V.HALF), "generic": set(V.MODES), "generic_feat": set(V.MODES),
                     "noviews": set(V.MODES)}
    for arm in modes:
        assert any(c["prefill"] for c in V.CASES if c["arm"] == arm), arm
    # every size class of every workgroup size, in every arm that runs more than one network size
    for arm in ("c", "pipe", "pipe_feat", "generic", "generic_feat", "noviews"):
        for m in modes[arm]:
            n = {c["R"] * c["S"] for c in V.CASES if c["arm"] == arm and c["mode"] == m and c["R"] is not None}
            assert n >= {1, 129, 259, 2310}, (arm, m, n)
    # the generic kernel: three widths, both direction-encoding forms, D = 1, the deepest network, a skip that feeds the last layer
    gen = {V.net_dims(c["net"])[:5] + (c["kind"],) for c in V.CASES if c["arm"] in ("generic", "generic_feat") and c["mode"] != "f16x3"}
    assert {g[1] for g in gen} == {64, 128, 256} and {g[3] > 4 for g in gen} == {False, True}
    assert (1, 64, 0, 0, None, 2) in gen and (2, 256, 10, 10, 0, 2) in gen and any(g[0] == 14 for g in gen)
    # what evd_nerf_mlp refuses
    assert V.expected_arm(V.case("x", "std", "f16c", 3, 43, kind=1)) is None
    assert V.expected_arm(V.case("x", "c", "f16c", 3, 43)) is None and V.expected_arm(V.case("x", "deep", "f16c", 3, 43)) is None
    assert V.expected_arm(V.case("x", "nv256o4", "f16c", 3, 43)) is None and V.expected_arm(V.case("x", "nv256o4", "f32", 3, 43, kind=1)) is None


def test_gains_touch_pts_linears_only_and_the_bias_block_holds_the_deep_network():
    for net, (D, Wd, L, Lv, skip, seed, gain, och) in V.NETS.items():
        sd = V.state_dict(net)
        ref = W.make_nerf_state_dict(seed, D, Wd, input_ch=W.pe_dim(L), input_ch_views=0 if och else W.pe_dim(Lv),
                                     skips=() if skip is None else (skip,), use_viewdirs=not och, output_ch=och or 4)
        assert list(sd) == list(ref)
        for k in sd:
            want = ref[k] * np.float32(gain) if (k.startswith("pts_linears.") and k.endswith(".weight")) else ref[k]
            assert sd[k].dtype == np.float32 and np.array_equal(sd[k], want), (net, k)
    assert "rgb_linear.bias" not in V.state_dict("std", False) and "rgb_linear.bias" in V.state_dict("std", True)
    nbias = lambda D, Wd: D * Wd + 32 + Wd + Wd // 2 + 32          # one 32-float block per output tile (evd_nerf_create)
    assert nbias(14, 256) <= 4096 < nbias(15, 256) and V.net_dims("deep")[:2] == (14, 256)


@pytest.mark.parametrize("net", ["nv256o4", "nv256o5", "nv64o4", "nv64o5", "std", "d", "f"])
def test_heads_and_feature_outputs_match_the_oracle(net):
    """output_linear (rows 0..3 of an output_ch 4 or 5 head) and the "before_linear" rows of a use_viewdirs=False network, which golden G40
    does not cover, against the oracle's Nerf / nerf_mlp (itself pinned to the reference by tests/test_oracle_golden.py): 1e-5 on float32
    inputs.  The view-branch networks: both feature outputs the same way."""
    from oracle import oracle as O
    D, Wd, L, Lv, skip, och = V.net_dims(net)
    R, S = 37, 7
    sd = V.state_dict(net)
    rb, z = V.inputs(R, S, 8 if och else 11)
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    emb = O.embed(pts, L)
    if not och:
        emb = np.concatenate([emb, O.embed(np.repeat(rb[:, None, 8:11], S, 1).reshape(-1, 3), Lv)], -1)
    onet = O.Nerf(sd, D=D, W=Wd, input_ch=W.pe_dim(L), input_ch_views=0 if och else W.pe_dim(Lv), skip=-1 if skip is None else skip,
                  use_viewdirs=not och, output_ch=och or 4)
    raw, fa, fb = O.nerf_mlp(onet, emb, want_after=not och, want_before=True)
    got = V.evaluate_net(net, R, S)
    assert got["raw"].shape == (R * S, 4) and got["feature2"].shape == (R * S, Wd)
    assert float(np.abs(got["raw"].numpy() - raw[:, :4]).max()) < 1e-5
    assert float(np.abs(got["feature2"].numpy() - fb).max()) < 1e-5
    if och:
        assert got["feature1"] is None and raw.shape == (R * S, 4)
        bad = V.evaluate_net(net, R, S, fault="out_swap")["raw"]
        assert float(np.abs(bad.numpy() - raw[:, :4]).max()) > 1e-2             # 1e-5 catches a wrong head
    else:
        assert float(np.abs(got["feature1"].numpy() - fa).max()) < 1e-5


def test_mode_model_differs_from_exact_by_the_type_s_resolution():
    ex = V.evaluate_net("std", 37, 7)
    for quant, lo, hi in (("f16", 1e-5, 2e-3), ("bf16", 1e-4, 2e-2)):
        qm = V.evaluate_net("std", 37, 7, quant=quant)
        for k in OUTS:
            assert lo < float((qm[k] - ex[k]).abs().max()) < hi, (quant, k)
