"""The cases of tests/test_gpu_bwd_walk.py can fail: the tile lists of the persistent backward kernels' workgroups against the table the
cases were designed from, and float64 autograd with one tile of a multi-tile workgroup dropped or counted twice against the bounds the
GPU test holds the kernels to.  The parameter gradients are linear in the incoming gradient, so the faulty sums are the reference itself
with that tile's d raw scaled by 0 or 2."""
import numpy as np
import pytest

import bwd_walk_ref as R


def _counts(tiles, blocks):
    return [len(t) for t in R.walk_split(tiles, blocks)]


def test_tile_lists_of_the_grid_stride_walk():
    # nsamp = 256 k - 83: 5 full tiles, one of 13 samples, 2 of padding in the last group of 8
    for n in (173, 429, 6317, 8365):
        t = R.tiles_of(n)
        assert t % 8 == 0 and [R.tile_samples(n, i) for i in range(t - 8, t)] == [32] * 5 + [13, 0, 0]
    # the table: EVD_BWD_OVERLAP -> (workgroups, tiles, tiles per workgroup)
    assert (R.nerf_blocks("1"), R.tiles_of(173), _counts(8, 1)) == (1, 8, [8])
    assert R.walk_split(8, R.nerf_blocks("3")) == [[0, 3, 6], [1, 4, 7], [2, 5]]
    assert (R.tiles_of(429), _counts(16, R.nerf_blocks("5"))) == (16, [4, 3, 3, 3, 3])
    assert R.walk_split(16, 5)[0] == [0, 5, 10, 15]
    assert _counts(8, R.nerf_blocks("7")) == [2, 1, 1, 1, 1, 1, 1] and R.walk_split(8, 7)[0] == [0, 7]
    assert (R.nerf_blocks(None), R.tiles_of(6317)) == (192, 200) and _counts(200, 192) == [2] * 8 + [1] * 184
    assert (R.nerf_blocks("0"), R.tiles_of(8365)) == (256, 264) and _counts(264, 256) == [2] * 8 + [1] * 248
    assert R.nerf_blocks("1000") == 256 and R.nerf_blocks("-3") == 256
    # the fine level: the NeRF trunk's count with EVD_BWD_OVERLAP_VOXEL, 256 without it or without a side stream
    assert [R.level_blocks(o, True) for o in ("1", "3", "5", "7", None, "0")] == [1, 3, 5, 7, 192, 256]
    assert all(R.level_blocks(o, False) == 256 for o in ("1", "7", None, "0"))
    for row in R.ROWS:
        for c in R.walk_cases(row[0]):
            assert c.sweep and all(R.tile_samples(c.nsamp, t) > 0 for t in c.sweep), c
            owner = [ts for ts in R.walk_split(R.tiles_of(c.nsamp), c.blocks) if c.sweep[0] in ts][0]
            assert len(owner) > 1 and set(c.sweep) <= set(owner), c
    assert R.walk_cases("1")[0].sweep == [0, 1, 2, 3, 4, 5] and R.walk_cases(None)[0].sweep[0] >= 192 and R.walk_cases("0")[1].sweep[0] >= 256


def test_pass_lists_of_the_four_wavefront_walk():
    i, ii = R.smallest_wave_cases()
    assert (i, R.tiles_of(i), ii, R.tiles_of(ii)) == (32941, 1032, 98221, 3072)
    sp = R.wave_split(1032)
    assert len(sp) == 256 and [len(p) for p in sp] == [2, 2] + [1] * 254
    assert sp[0][1] == [1024, 1025, 1026, 1027] and sp[1] == [[4, 5, 6, 7], [1028, 1029, 1030, 1031]]
    assert [R.tile_samples(i, t) for t in sp[1][1]] == [32, 13, 0, 0]                 # two live wavefronts in workgroup 1's second pass
    assert R.tiles_of(R.nsamp_of(128)) == 1024 and all(len(p) == 1 for p in R.wave_split(1024))
    sp = R.wave_split(3072)
    assert all(len(p) == 3 for p in sp) and sp[255][2] == [3068, 3069, 3070, 3071] and any(len(p) < 3 for p in R.wave_split(3064))
    assert R.wave_split(5) == [[[0, 1, 2, 3]], [[4]]]
    # the per-layer chain's wgrads on the same stores: every workgroup 4 or 5 tiles, then 12
    assert R.split_summary(_counts(1032, 256)) == "8 x 5, 248 x 4" and R.split_summary(_counts(3072, 256)) == "256 x 12"
    # the reduced sample sets of the discrimination test below have the same shapes with 3 workgroups
    a, b = R.smallest_wave_cases(3)
    assert (a, b) == (429, 1197)
    assert [len(p) for p in R.wave_split(R.tiles_of(a), 3)] == [2, 1, 1] and [R.tile_samples(a, t) for t in R.wave_split(16, 3)[0][1]] == [32, 13, 0, 0]
    assert [len(p) for p in R.wave_split(R.tiles_of(b), 3)] == [4, 3, 3]
    for c in R.wave_cases() + R.reduced_wave_cases():
        grid = min(R.tiles_of(c.nsamp) // 4, c.blocks)
        assert c.sweep[0] == 4 * grid and R.tile_samples(c.nsamp, c.sweep[1]) == 13, c


def test_relu_ties_of_the_float32_grade_cases_stay_under_the_cap():
    """f16x3 is held to the true ReLU pattern; where a case misses its bound as drawn, d raw is zeroed on the samples that hold a
    pre-activation within TAU of zero (tests/bwd_walk_driver.py): at most TIE_CAP of any case's samples"""
    sd = R.state_dict("nerf")
    for row in R.ROWS:
        case = R.walk_cases(row[0])[0]
        share = float(R.nerf_tie_samples(sd, R.case_inputs(case)).mean())
        print(f"[{case.name}, tiles {case.sweep} swept] samples with a ReLU tie: {share:.2%}")
        assert share <= R.TIE_CAP, (case, share)


def _all_cases():
    seen, out = set(), []
    for row in R.ROWS:
        for c in R.walk_cases(row[0]):
            if (c.net, c.nsamp, tuple(c.sweep)) not in seen:
                seen.add((c.net, c.nsamp, tuple(c.sweep)))
                out.append((f"{c.name}-overlap_{'unset' if row[0] is None else row[0]}", c))
    return out + [(c.name + "-reduced", c) for c in R.reduced_wave_cases()]


_CASES = _all_cases()


@pytest.mark.parametrize("case", [c for _, c in _CASES], ids=[i for i, _ in _CASES])
def test_a_dropped_or_repeated_tile_fails_the_case(case):
    """every swept tile of the case, dropped (d raw x 0) or counted twice (x 2): every parameter gradient moves by at least 10 x the
    loosest bound the case is held to (bf16: 3e-2)"""
    sd, inp = R.state_dict(case.net), R.case_inputs(case)
    full = R.reference_chunked(case, sd, inp)
    bound = max(R.TOL[p] for p in (R.NERF_PRECS if case.net == "nerf" else R.LEVEL_PRECS))
    margin = {}
    for t in case.sweep:
        lo, hi = 32 * t, min(32 * t + 32, case.nsamp)
        own = R.reference(case, sd, inp, rows=slice(lo, hi))                # the tile's own contribution: the sums are linear in d raw
        for s in (0.0, 2.0):
            if case.nsamp <= 1200:                                           # the small cases: the faulty sum itself, by autograd
                wrong = R.reference(case, sd, R.scale_tile(inp, t, s))
            else:
                wrong = {k: full[k] + (s - 1.0) * own[k] for k in full if R.is_param(k)}
            for k in full:
                if R.is_param(k):
                    if case.nsamp <= 1200:
                        assert np.allclose(wrong[k], full[k] + (s - 1.0) * own[k], rtol=1e-9, atol=1e-12 * np.abs(full[k]).max()), (k, t, s)
                    moved = R.rel_l2(wrong[k], full[k])
                    margin[k] = min(margin.get(k, np.inf), moved / bound)
    worst = min(margin, key=margin.get)
    print(f"[{case.name}: tiles {case.sweep} of {R.tiles_of(case.nsamp)}] smallest movement of a parameter gradient / bound {bound:g}: "
          f"{margin[worst]:.1f} ({worst})")
    assert margin[worst] >= 10.0, {k: f"{v:.1f}" for k, v in sorted(margin.items(), key=lambda kv: kv[1])[:6]}
