"""The training backward where a workgroup of a persistent kernel walks SEVERAL sample tiles, against float64 autograd.

tests/test_gpu_train.py, test_gpu_awp.py and test_gpu_train_f32grade.py hold these kernels to float64 with one tile per workgroup; here
the grid-stride loops run: the 3-deep LDS-DMA ring with its counted waits, the slot rotation, the exchange-buffer parity and the prologue
that issues past the last tile (k_wgrad, k_wgrad_split, k_wgrad_dgrad), the fold of k_wgrad_reduce over 1, 3, 5, 7 partials, and the
second and third passes of k_voxel_bwd_fused64 / k_awp_bwd_fused.  EVD_BWD_OVERLAP (with the side stream on: the number of persistent
wgrad workgroups) is read once per process, so every row of bwd_walk_ref.ROWS but the shipped one runs tests/bwd_walk_driver.py in a
child process; the children run one after another, a non-zero exit, a signal or the time limit fails the test.

Per case: every parameter gradient and every input gradient within the project's float64 bounds (4e-3 f16, 3e-2 bf16 with the kernel's
own ReLU pattern; 5e-6 f16x3 with the true one), every output finite, a second backward on the same store bit-identical in the
per-sample outputs; the small rows also against the same inputs at one tile per workgroup (EVD_BWD_OVERLAP=0): parameter gradients within
1e-5 (float32 partial sums in another order), per-sample gradients bit for bit.  tests/test_bwd_walk_ref.py shows on the CPU that a
dropped or repeated tile fails these cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bwd_walk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every switch that selects a backward form or grid (evd_common.h bwd_overlap_blocks, BwdSwitches): none may reach a case from outside
SWITCHES = ("EVD_BWD_OVERLAP", "EVD_BWD_OVERLAP_VOXEL", "EVD_AWP_BWD_FUSE", "EVD_BWD_FUSE64", "EVD_BWD_FUSE_SG", "EVD_BWD_YGEN", "EVD_BWD_ROWS")
pytestmark = pytest.mark.gpu


def _spec(case, tag, prec, **kw):
    return dict(name=f"{case.name}@{tag}", net=case.net, nsamp=case.nsamp, blocks=case.blocks, sweep=case.sweep, prec=prec, **kw)


def _row_specs(overlap, tag, keep):
    nerf, fine = R.walk_cases(overlap)
    return [_spec(nerf, tag, p, keep=keep) for p in R.NERF_PRECS] + [_spec(fine, tag, p, keep=keep) for p in R.LEVEL_PRECS]


def _specs(run):
    """the cases of one process: a row of the table; "0" also runs the small rows' inputs at one tile per workgroup; "chain": the AWP
    embedding's per-layer chain (EVD_AWP_BWD_FUSE=0) on the cases of (b); "wave": the fused forms of (b), no switch"""
    if run == "wave":
        return [_spec(c, "wave", p) for c in R.wave_cases() for p in R.LEVEL_PRECS]
    if run == "chain":
        return [_spec(c, "chain", p) for c in R.wave_cases() if c.net == "awp" for p in R.LEVEL_PRECS]
    tag = "unset" if run is None else run
    specs = _row_specs(run, tag, keep=run in R.SMALL_ROWS)
    if run == "3":          # one trunk layer's gradient pointers null: the per-layer path (k_wgrad skipped, k_dgrad_layer) inside the fused chain
        specs.append(_spec(R.walk_cases(run)[0], tag, "f16", null_layers=[5, 7]))
    if run == "0":
        for small in R.SMALL_ROWS:
            specs += [dict(s, name=s["name"] + "/one", blocks=256) for s in _row_specs(small, small, keep=True)]
    return specs


def _env(run):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if run == "chain":
        env["EVD_AWP_BWD_FUSE"] = "0"
    elif run in R.SMALL_ROWS:
        env["EVD_BWD_OVERLAP"], env["EVD_BWD_OVERLAP_VOXEL"] = run, "1"
    elif run == "0":
        env["EVD_BWD_OVERLAP"] = "0"
    return env


_done = {}


def _results(run, tmp_path_factory):
    """the arrays of one process, run ONCE per session whatever its end: a child that exits non-zero, dies on a signal or runs into the time
    limit is not started again -- every later test that needs it fails at once with the first failure.  The shipped settings need no
    child unless the environment sets a switch"""
    if run not in _done:
        try:
            _done[run] = _run_once(run, tmp_path_factory)
        except BaseException as e:          # (the time limit and a keyboard interrupt included: nothing of this run starts twice)
            _done[run] = e
            raise
    if isinstance(_done[run], BaseException):
        raise AssertionError(f"the cases of run {run!r} failed in an earlier test and are not started again: {_done[run]}")
    return _done[run]


def _run_once(run, tmp_path_factory):
    specs = _specs(run)
    if run in (None, "wave") and not any(k in os.environ for k in SWITCHES):
        import bwd_walk_driver
        return bwd_walk_driver.run_cases(specs)
    d = tmp_path_factory.mktemp("bwd_walk")
    cases, out = str(d / "cases.json"), str(d / "out.npz")
    with open(cases, "w") as f:
        json.dump(specs, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bwd_walk_driver.py"), cases, out], env=_env(run), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"the driver ended with {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout, end="")
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def _check_float64(res, specs):
    """-> {case key: (worst error / bound, tensor)}; asserts the bounds, finiteness, the repeated backward and the sentinels"""
    worst = {}
    for s in specs:
        key = f"{s['name']}.{s['prec']}" + (".null" if s.get("null_layers") else "")
        errs = {k[len(key) + 5:]: float(v) for k, v in res.items() if k.startswith(key + "/err/")}
        assert errs, key
        assert res[key + "/finite"] == 1, key
        assert res[key + "/repeat"] == 1, f"{key}: a second backward on the same store changed a per-sample output"
        for k, v in res.items():
            if k.startswith(key + "/sentinel/"):
                assert v == 1, f"{k}: a gradient buffer behind a null pointer was written"
        if s.get("null_layers"):
            assert sum(k.startswith(key + "/sentinel/") for k in res) == 2 * len(s["null_layers"]) and len(errs) == 24 - 2 * len(s["null_layers"]) + 2
        name = max(errs, key=lambda k: errs[k] / R.tol(s["net"], s["prec"], k))
        worst[key] = (errs[name] / R.tol(s["net"], s["prec"], name), name, errs[name])
        bad = {k: f"{v:.2e}" for k, v in errs.items() if not v < R.tol(s["net"], s["prec"], k)}
        assert not bad, f"{key} ({s['nsamp']} samples, at most {s['blocks']} workgroups): relative L2 against float64 autograd beyond the bound: {bad}"
    return worst


@pytest.mark.parametrize("run", ["1", "3", "5", "7", None, "0"], ids=lambda r: f"overlap_{'unset' if r is None else r}")
def test_multi_tile_walk_matches_float64_autograd(run, tmp_path_factory):
    """(a): NeRF 8 x 256 in f16 / bf16 / f16x3 and the fine PDRF level in f16 / bf16 on one row of the table.  Measured: f16 below 0.6,
    bf16 below 0.65 and f16x3 below 0.2 of their bounds on every row.  f16x3 at 8365 samples (EVD_BWD_OVERLAP=0) as drawn: 1.5e-3 in
    pts_linears.0-3 only, and 1.9e-3 on its first 6144 samples at one tile per workgroup -- ReLU ties, not the walk; with d raw zeroed on the
    3.75 % of samples that hold a float64 pre-activation within TAU of zero: 7.8e-7 (bwd_walk_driver.run_cases).  The f16x3 per-sample
    gradients d_pts / d_dirs: at most 2.9e-7 / 2.0e-7 on every row"""
    specs = [s for s in _specs(run) if not s["name"].endswith("/one")]
    for c in R.walk_cases(run):
        sp = R.walk_split(R.tiles_of(c.nsamp), c.blocks)
        print(f"[{c.name}, EVD_BWD_OVERLAP {'unset' if run is None else run}] {R.tiles_of(c.nsamp)} tiles on {len(sp)} workgroups, "
              f"workgroups x tiles: {R.split_summary([len(t) for t in sp])}")
    worst = _check_float64(_results(run, tmp_path_factory), specs)
    for key, (ratio, name, err) in worst.items():
        print(f"  {key}: worst relative L2 vs float64 {err:.2e} ({name}), {ratio:.2f} of its bound")


@pytest.mark.parametrize("run", list(R.SMALL_ROWS), ids=lambda r: f"overlap_{r}")
def test_multi_tile_walk_equals_one_tile_per_workgroup(run, tmp_path_factory):
    """the same inputs at EVD_BWD_OVERLAP=0 (256 workgroups: one tile each, the form the one-tile float64 tests pin): the parameter gradients
    differ in the order of float32 partial sums only, the per-sample gradients are formed tile by tile and do not depend on the grid"""
    walk, one = _results(run, tmp_path_factory), _results("0", tmp_path_factory)
    worst = {}
    for s in _row_specs(run, run, True):
        key = f"{s['name']}.{s['prec']}"
        names = [k[len(key) + 3:] for k in walk if k.startswith(key + "/g/")]
        assert names, key
        for name in names:
            a, b = walk[f"{key}/g/{name}"], one[f"{s['name']}/one.{s['prec']}/g/{name}"]
            if R.is_param(name):
                e = R.rel_l2(a, b)
                worst[key] = max(worst.get(key, 0.0), e)
                assert e < R.CROSS_GRID_TOL, (key, name, e)
            else:
                diff = np.flatnonzero(a.reshape(-1).view(np.uint32) != b.reshape(-1).view(np.uint32))
                assert diff.size == 0, f"{key} {name}: {diff.size} words differ between the grids, first at {diff[0]}"
    print(f"[EVD_BWD_OVERLAP={run} vs 0] worst relative L2 of a parameter gradient across the grids:", {k: f"{v:.1e}" for k, v in worst.items()})


@pytest.mark.parametrize("run", ["wave", "chain"])
def test_fused_chain_passes_match_float64_autograd(run, tmp_path_factory):
    """(b): no switch sets the grid of k_voxel_bwd_fused64, k_awp_bwd_fused or the AWP per-layer chain (min(tiles / 4, 256) and
    min(tiles, 256) workgroups), so the second and third passes need sample counts beyond 256 x 4 tiles"""
    for n in R.smallest_wave_cases():
        tiles = R.tiles_of(n)
        sp = R.wave_split(tiles)
        live2 = sorted({sum(R.tile_samples(n, t) > 0 for t in p[1]) for p in sp if len(p) > 1})
        print(f"[{n} samples] {tiles} tiles; fused forms: {len(sp)} workgroups x passes {R.split_summary([len(p) for p in sp])}, live wavefronts in a "
              f"second pass {live2}; per-layer wgrads: workgroups x tiles {R.split_summary([len(t) for t in R.walk_split(tiles, 256)])}")
    worst = _check_float64(_results(run, tmp_path_factory), _specs(run))
    for key, (ratio, name, err) in worst.items():
        print(f"  {key}: worst relative L2 vs float64 {err:.2e} ({name}), {ratio:.2f} of its bound")
