"""CPU-only checks of the LPIPS path: the float64 yardstick tests/lpips_ref.py against golden G38 (the reference's real LPIPS class in
.double(), tools/gen_golden.py G38_lpips), the state-dict validation of metrics.LPIPS, the argument validation of evd_lpips (before the
device is touched) and the set_lpips switch of compute_img_metric.

The 1e-10 bound on the restatement: both sides are float64 on the same float32-valued inputs and weights; they differ in summation order only
(explicit patches and one matrix product here, torch's convolution there), i.e. by ~sqrt(K) 2^-53 ~ 1e-14 per feature."""
import ctypes

import numpy as np
import pytest

import lpips_ref as R
from conftest import load_golden
from evdeblurnerf_amd import weights as W


@pytest.fixture(scope="module")
def g38():
    return load_golden("G38_lpips")


def g38_inputs(g, tag):
    B, H, Wd, seed = (int(v) for v in g[tag + ".args"])
    lo, hi = (float(v) for v in g[tag + ".range"])
    return W.synthetic_frame_pairs(seed, B, H, Wd, lo, hi)


def g38_weights(g):
    return W.make_lpips_alexnet_state_dict(int(g["backbone_seed"])), [g[f"lin{l}"] for l in range(5)]


def test_fixture_holds_the_cases_and_the_heads(g38):
    cases = {str(c): tuple(int(v) for v in g38[str(c) + ".args"][:3]) for c in g38["cases"]}
    assert (2, 31, 31) in cases.values() and (2, 35, 47) in cases.values() and (1, 67, 90) in cases.values()
    assert any(g38[c + ".range"][0] < 0 and g38[c + ".range"][1] > 1 for c in cases)            # one case leaves (0, 1)
    assert [g38[f"lin{l}"].size for l in range(5)] == [64, 192, 384, 256, 256]
    assert all((g38[f"lin{l}"] >= 0).all() for l in range(5))
    for c in cases:
        assert np.allclose(g38[c + ".f64.terms"].sum(axis=1), g38[c + ".f64.value"], rtol=1e-12)      # per-layer terms, not the in-place total
        assert 0 < g38[c + ".ref_f32_err.value"].max() < 1e-5 and 0 < g38[c + ".ref_f32_err.terms"].max() < 1e-4


def test_restatement_reproduces_the_float64_reference(g38):
    backbone, lins = g38_weights(g38)
    for c in (str(c) for c in g38["cases"]):
        pred, target = g38_inputs(g38, c)
        value, terms = R.lpips(pred, target, backbone, lins, g38["shift"], g38["scale"])
        ev = np.abs(value - g38[c + ".f64.value"]) / g38[c + ".f64.value"]
        et = np.abs(terms - g38[c + ".f64.terms"]) / g38[c + ".f64.terms"]
        print(f"{c}: value {ev.max():.1e}, terms {et.max():.1e}")
        assert ev.max() <= 1e-10 and et.max() <= 1e-10, (c, ev, et)


def test_restatement_clamp_and_zero_features(g38):
    backbone, lins = g38_weights(g38)
    pred, target = g38_inputs(g38, "clamp")
    v0, _ = R.lpips(pred, target, backbone, lins, g38["shift"], g38["scale"])
    v1, _ = R.lpips(np.clip(pred, 0, 1), np.clip(target, 0, 1), backbone, lins, g38["shift"], g38["scale"])
    assert np.array_equal(v0, v1)                                # clamp(2 x - 1, -1, 1) == 2 clip(x, 0, 1) - 1 in float32
    dead = {k: (np.full_like(v, -10.0) if k.endswith("bias") else v) for k, v in backbone.items()}
    v, t = R.lpips(pred, target, dead, lins, g38["shift"], g38["scale"])
    assert np.array_equal(v, np.zeros_like(v)) and np.array_equal(t, np.zeros_like(t))


def test_state_dict_validation_names_the_key(g38):
    from evdeblurnerf_amd import _lib
    from evdeblurnerf_amd.metrics import LPIPS
    backbone, lins = g38_weights(g38)
    heads = {f"lin{l}.model.1.weight": lins[l].reshape(1, -1, 1, 1) for l in range(5)}
    missing = {k: v for k, v in backbone.items() if k != "features.6.bias"}
    with pytest.raises(_lib.EvdError, match=r"features\.6\.bias"):
        LPIPS(missing, heads)
    bad = dict(backbone)
    bad["features.3.weight"] = np.zeros((192, 64, 3, 3), np.float32)
    with pytest.raises(_lib.EvdError, match=r"features\.3\.weight"):
        LPIPS(bad, heads)
    with pytest.raises(_lib.EvdError, match=r"lin4\.model\.1\.weight"):
        LPIPS(backbone, {k: v for k, v in heads.items() if not k.startswith("lin4")})
    short = dict(heads)
    short["lin2.model.1.weight"] = np.zeros((1, 256, 1, 1), np.float32)
    with pytest.raises(_lib.EvdError, match=r"lin2\.model\.1\.weight"):
        LPIPS(backbone, short)


def test_lpips_argument_validation_without_gpu():
    """evd_lpips validates before it touches the device or the handle: callable on a CPU-only box (the non-null arguments below are host
    buffers nobody dereferences)."""
    from evdeblurnerf_amd import build, _lib
    build.build()
    h = _lib.lib()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(dummy))
    need = h.evd_lpips_workspace_bytes(2, 31, 31)
    assert need > 0 and h.evd_lpips_workspace_bytes(8, 400, 400) > need
    for bad in ((0, 31, 31), (1, 30, 64), (1, 64, 30)):
        assert h.evd_lpips_workspace_bytes(*bad) == 0, bad
    assert h.evd_lpips(p, p, p, 1, 30, 64, p, p, 1 << 30, None) == -1 and b"31" in h.evd_last_error()
    assert h.evd_lpips(p, p, p, 1, 64, 30, p, p, 1 << 30, None) == -1 and b"evd_lpips" in h.evd_last_error()
    assert h.evd_lpips(p, p, p, 0, 31, 31, p, p, 1 << 30, None) == -1 and b"B=0" in h.evd_last_error()
    for nulls in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        m, a, b, o, ws = nulls
        assert h.evd_lpips(m, a, b, 2, 31, 31, o, ws, need, None) == -1, nulls
        assert b"evd_lpips" in h.evd_last_error()
    assert h.evd_lpips(p, p, p, 2, 31, 31, p, p, need - 1, None) == -1 and b"workspace" in h.evd_last_error()
    assert h.evd_lpips_create(None, None) == -1 and b"evd_lpips_create" in h.evd_last_error()
    desc = _lib.LpipsDesc()                                      # every weight pointer null
    out = ctypes.c_void_p()
    assert h.evd_lpips_create(ctypes.byref(desc), ctypes.byref(out)) == -1 and not out.value
    h.evd_lpips_destroy(None)


def test_set_lpips_switch():
    from evdeblurnerf_amd import _lib
    from evdeblurnerf_amd import metrics as M

    class Stub(M.LPIPS):
        def __init__(self):
            pass

        def mean(self, im1, im2, format=None):
            return 0.25

    try:
        M.set_lpips(Stub())
        assert M.compute_img_metric(None, None, "lpips", margin=0.1, mask=object()) == 0.25       # margin and mask never reach the model
        with pytest.raises(_lib.EvdError):
            M.set_lpips(object())
    finally:
        M.set_lpips(None)
    with pytest.raises(NotImplementedError, match="weights"):
        M.compute_img_metric(None, None, "lpips")
