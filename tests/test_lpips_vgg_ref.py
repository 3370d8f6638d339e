"""CPU-only checks of the LPIPS options beyond the reference's default call: the float64 yardstick tests/lpips_vgg_ref.py against golden
G43 (the reference's real LPIPS class with net='vgg' in .double(): heads and baseline, spatial average and spatial map, version 0.0;
tools/gen_golden.py G43_lpips_vgg) and, for AlexNet, against G38 and tests/lpips_ref.py; the argument validation of the new C entries
(before the device is touched) and of the metrics.LPIPS constructor.

The 1e-10 bound on the restatement: both sides are float64 on the same float32-valued inputs and weights; they differ in summation order only
(explicit patches and one matrix product here, torch's convolution there), i.e. by ~sqrt(K) 2^-53 ~ 1e-14 per feature, through 13 layers.
Values and terms are compared relatively, a map by its largest absolute error over its largest value (a map has pixels near 0)."""
import ctypes

import numpy as np
import pytest

import lpips_ref as R
import lpips_vgg_ref as RV
from conftest import load_golden
from evdeblurnerf_amd import weights as W

VARIANTS = {"": dict(heads=True, v00=False), "base.": dict(heads=False, v00=False), "v00.": dict(heads=True, v00=True)}


@pytest.fixture(scope="module")
def g43():
    return load_golden("G43_lpips_vgg")


def g43_inputs(g, tag):
    B, H, Wd, seed = (int(v) for v in g[tag + ".args"])
    lo, hi = (float(v) for v in g[tag + ".range"])
    return W.synthetic_frame_pairs(seed, B, H, Wd, lo, hi)


def g43_setup(g, heads=True, v00=False):
    """backbone, lins, shift, scale of a variant"""
    lins = [g[f"lin{l}"] for l in range(5)] if heads else None
    shift, scale = (np.zeros(3, np.float32), np.ones(3, np.float32)) if v00 else (g["shift"], g["scale"])
    return W.make_lpips_vgg16_state_dict(int(g["backbone_seed"])), lins, shift, scale


def map_err(got, want):
    """largest absolute error over the largest value, per leading index (image, or image and layer)"""
    ax = (-2, -1)
    return np.abs(got - want).max(axis=ax) / np.abs(want).max(axis=ax)


def test_fixture_holds_the_cases_and_the_heads(g43):
    cases = {str(c): tuple(int(v) for v in g43[str(c) + ".args"][:3]) for c in g43["cases"]}
    assert len(cases) >= 6
    for shape in ((1, 16, 16), (1, 16, 33), (1, 33, 16), (3, 37, 50), (2, 40, 56)):
        assert shape in cases.values(), shape
    assert any(g43[c + ".range"][0] < 0 and g43[c + ".range"][1] > 1 for c in cases)            # one case leaves (0, 1)
    assert [g43[f"lin{l}"].size for l in range(5)] == [64, 128, 256, 512, 512]
    assert all((g43[f"lin{l}"] >= 0).all() for l in range(5))
    assert str(g43["v00_case"]) in cases
    for c in cases:
        B, H, Wd = cases[c]
        for pre in ("", "base."):
            k = c + "." + pre
            assert np.allclose(g43[k + "f64.terms"].sum(axis=1), g43[k + "f64.value"], rtol=1e-12)    # per-layer terms, not the in-place total
            assert g43[k + "f64.terms"].min() > 1e-6
            assert 0 < g43[k + "ref_f32_err.value"].max() < 1e-5 and 0 < g43[k + "ref_f32_err.terms"].max() < 1e-4
            assert g43[k + "f64.map"].shape == (B, H, Wd) and g43[k + "ref_f32_err.map"].shape == (B,)
            assert 0 < g43[k + "ref_f32_err.map"].max() < 1e-4


def test_restatement_reproduces_the_float64_reference(g43):
    n_layer_maps = 0
    for c in (str(c) for c in g43["cases"]):
        pred, target = g43_inputs(g43, c)
        for pre, kw in VARIANTS.items():
            k = c + "." + pre
            if k + "f64.value" not in g43:
                assert pre == "v00."
                continue
            setup = g43_setup(g43, **kw)
            value, terms = RV.lpips(pred, target, *setup, net="vgg")
            smap, layers = RV.lpips_spatial(pred, target, *setup, net="vgg")
            ev = np.abs(value - g43[k + "f64.value"]) / g43[k + "f64.value"]
            et = np.abs(terms - g43[k + "f64.terms"]) / g43[k + "f64.terms"]
            em = map_err(smap, g43[k + "f64.map"])
            print(f"{k[:-1]}: value {ev.max():.1e}, terms {et.max():.1e}, map {em.max():.1e}")
            assert ev.max() <= 1e-10 and et.max() <= 1e-10 and em.max() <= 1e-10, (k, ev, et, em)
            if k + "f64.layer_maps" in g43:
                el = map_err(layers, g43[k + "f64.layer_maps"])
                assert el.max() <= 1e-10, (k, el)
                n_layer_maps += 1
    assert n_layer_maps >= 6 and str(g43["v00_case"]) + ".v00.f64.layer_maps" in g43


def test_restatement_on_alexnet_agrees_with_lpips_ref():
    """the table-driven restatement with net='alex' is tests/lpips_ref.py (held to G38); its map averages to the value where no resampling
    is involved"""
    g38 = load_golden("G38_lpips")
    backbone, lins = W.make_lpips_alexnet_state_dict(int(g38["backbone_seed"])), [g38[f"lin{l}"] for l in range(5)]
    B, H, Wd, seed = (int(v) for v in g38["odd.args"])
    pred, target = W.synthetic_frame_pairs(seed, B, H, Wd)
    value, terms = RV.lpips(pred, target, backbone, lins, g38["shift"], g38["scale"], net="alex")
    assert np.allclose(value, g38["odd.f64.value"], rtol=1e-10, atol=0) and np.allclose(terms, g38["odd.f64.terms"], rtol=1e-10, atol=0)
    v2, t2 = R.lpips(pred, target, backbone, lins, g38["shift"], g38["scale"])
    assert np.allclose(value, v2, rtol=1e-13, atol=0) and np.allclose(terms, t2, rtol=1e-13, atol=0)
    base, _ = RV.lpips(pred, target, backbone, None, g38["shift"], g38["scale"], net="alex")
    ones, _ = RV.lpips(pred, target, backbone, [np.ones(c, np.float32) for c in (64, 192, 384, 256, 256)], g38["shift"], g38["scale"], net="alex")
    assert np.array_equal(base, ones)                            # the baseline is heads of exact ones


def test_upsample_formula():
    import torch
    d = torch.arange(6, dtype=torch.float64).reshape(1, 2, 3)
    assert torch.equal(RV.upsample(d, 2, 3), d)                  # same size: the identity
    up = RV.upsample(d, 4, 3)[0, :, 0]                           # rows: s = max((o + 0.5) / 2 - 0.5, 0) = 0, 0.25, 0.75, 1.25 -> clamped neighbour
    assert np.allclose(up.numpy(), [0.0, 0.75, 2.25, 3.0], rtol=1e-15)
    one = torch.full((2, 1, 1), 0.5, dtype=torch.float64)
    assert torch.equal(RV.upsample(one, 5, 7), torch.full((2, 5, 7), 0.5, dtype=torch.float64))
    dead = RV.pool(torch.arange(25, dtype=torch.float64).reshape(1, 1, 5, 5), 2, 2)
    assert dead.shape == (1, 1, 2, 2) and dead.flatten().tolist() == [6.0, 8.0, 16.0, 18.0]      # floor: the last row and column are dropped


def test_new_entries_validate_without_gpu():
    """evd_lpips_create_net, evd_lpips_min_side, evd_lpips_model_workspace_bytes and evd_lpips_spatial validate before they touch the device:
    callable on a CPU-only box (the non-null arguments below are host buffers nobody dereferences beyond the handle's backbone id)."""
    from evdeblurnerf_amd import build, _lib
    build.build()
    h = _lib.lib()
    out = ctypes.c_void_p()
    assert h.evd_lpips_create_net(None, ctypes.byref(out)) == -1 and b"evd_lpips_create_net" in h.evd_last_error()
    desc = _lib.LpipsNetDesc()
    assert h.evd_lpips_create_net(ctypes.byref(desc), None) == -1 and b"null" in h.evd_last_error()
    desc.net = 7
    assert h.evd_lpips_create_net(ctypes.byref(desc), ctypes.byref(out)) == -1 and b"unknown backbone 7" in h.evd_last_error()
    keep = [np.zeros(512 * 512 * 9, np.float32)]
    fp = ctypes.cast(keep[0].ctypes.data, _lib._fp)
    desc.net, desc.heads = _lib.LPIPS_NET_VGG16, 1
    for l in range(13):
        desc.conv_w[l] = desc.conv_b[l] = fp
    for c in range(3):
        desc.scale[c] = 1.0
    for l in range(4):
        desc.lin[l] = fp                                         # head 4 stays null
    assert h.evd_lpips_create_net(ctypes.byref(desc), ctypes.byref(out)) == -1 and not out.value
    assert b"vgg16" in h.evd_last_error() and b"head 4" in h.evd_last_error()
    desc.conv_b[12] = None
    assert h.evd_lpips_create_net(ctypes.byref(desc), ctypes.byref(out)) == -1 and b"convolution 12" in h.evd_last_error()

    assert h.evd_lpips_min_side(_lib.LPIPS_NET_VGG16) == 16 and h.evd_lpips_min_side(_lib.LPIPS_NET_ALEX) == 31
    assert h.evd_lpips_min_side(2) == 0 and h.evd_lpips_min_side(-1) == 0
    assert h.evd_lpips_model_workspace_bytes(None, 2, 64, 64, 0) == 0 and h.evd_lpips_model_workspace_bytes(None, 2, 64, 64, 1) == 0

    # a host stand-in for a handle: only its first int, the backbone id, is read before the sizes are validated
    vgg = (ctypes.c_int * 16)(_lib.LPIPS_NET_VGG16)
    alex = (ctypes.c_int * 16)(_lib.LPIPS_NET_ALEX)
    pv, pa = ctypes.c_void_p(ctypes.addressof(vgg)), ctypes.c_void_p(ctypes.addressof(alex))
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(dummy))
    need = h.evd_lpips_model_workspace_bytes(pv, 2, 16, 16, 0)
    assert need >= 2 * (2 * 2 * 16 * 16 * 64) * 4                # two buffers of conv1_x: 2 B H W 64 floats each
    assert h.evd_lpips_model_workspace_bytes(pv, 2, 16, 16, 1) > need
    assert h.evd_lpips_model_workspace_bytes(pa, 2, 31, 31, 0) == h.evd_lpips_workspace_bytes(2, 31, 31)
    for bad in ((0, 16, 16), (1, 15, 64), (1, 64, 15), (1, 40000, 40000)):
        assert h.evd_lpips_model_workspace_bytes(pv, *bad, 0) == 0 and h.evd_lpips_model_workspace_bytes(pv, *bad, 1) == 0, bad
    assert h.evd_lpips_model_workspace_bytes(pa, 1, 30, 64, 1) == 0
    big = 1 << 40
    assert h.evd_lpips(pv, p, p, 1, 15, 64, p, p, big, None) == -1 and b"vgg16" in h.evd_last_error() and b"16" in h.evd_last_error()
    assert h.evd_lpips_spatial(pv, p, p, 1, 64, 15, p, None, p, big, None) == -1 and b"evd_lpips_spatial: vgg16" in h.evd_last_error()
    assert h.evd_lpips_spatial(pa, p, p, 1, 30, 64, p, None, p, big, None) == -1 and b"alex" in h.evd_last_error() and b"31" in h.evd_last_error()
    assert h.evd_lpips_spatial(pv, p, p, 0, 16, 16, p, None, p, big, None) == -1 and b"B=0" in h.evd_last_error()
    assert h.evd_lpips_spatial(pv, p, p, 1, 40000, 40000, p, None, p, big, None) == -1 and b"too large" in h.evd_last_error()
    for nulls in ((None, p, p, p, p), (pv, None, p, p, p), (pv, p, None, p, p), (pv, p, p, None, p), (pv, p, p, p, None)):
        m, a, b, o, ws = nulls
        assert h.evd_lpips_spatial(m, a, b, 2, 16, 16, o, None, ws, big, None) == -1, nulls
        assert b"evd_lpips_spatial" in h.evd_last_error()
    need = h.evd_lpips_model_workspace_bytes(pv, 2, 16, 16, 1)
    assert h.evd_lpips_spatial(pv, p, p, 2, 16, 16, p, None, p, need - 1, None) == -1 and b"workspace" in h.evd_last_error()


def test_constructor_validation(g43):
    from evdeblurnerf_amd import _lib
    from evdeblurnerf_amd.metrics import LPIPS
    backbone, lins, _, _ = g43_setup(g43)
    heads = {f"lin{l}.model.1.weight": lins[l].reshape(1, -1, 1, 1) for l in range(5)}
    with pytest.raises(NotImplementedError, match="fire modules"):
        LPIPS(backbone, heads, net="squeeze")
    with pytest.raises(_lib.EvdError, match="version"):
        LPIPS(backbone, heads, net="vgg", version="0.2")
    with pytest.raises(_lib.EvdError, match="net 'resnet'"):
        LPIPS(backbone, heads, net="resnet")
    with pytest.raises(_lib.EvdError, match="lin"):
        LPIPS(backbone, net="vgg")                               # lpips=True needs the heads
    missing = {k: v for k, v in backbone.items() if k != "features.28.bias"}
    with pytest.raises(_lib.EvdError, match=r"VGG-16 state dict has no 'features\.28\.bias'"):
        LPIPS(missing, heads, net="vgg16")
    bad = dict(backbone)
    bad["features.5.weight"] = np.zeros((128, 64, 5, 5), np.float32)
    with pytest.raises(_lib.EvdError, match=r"features\.5\.weight"):
        LPIPS(bad, heads, net="vgg")
    short = dict(heads)
    short["lin3.model.1.weight"] = np.zeros((1, 256, 1, 1), np.float32)      # AlexNet's width
    with pytest.raises(_lib.EvdError, match=r"lin3\.model\.1\.weight"):
        LPIPS(backbone, short, net="vgg")


def test_set_lpips_refuses_a_spatial_model():
    from evdeblurnerf_amd import _lib
    from evdeblurnerf_amd import metrics as M

    class Stub(M.LPIPS):
        def __init__(self, spatial):
            self.spatial = spatial

    with pytest.raises(_lib.EvdError, match="spatial"):
        M.set_lpips(Stub(True))
    with pytest.raises(_lib.EvdError, match="spatial"):
        Stub(True).mean(None, None)
    try:
        M.set_lpips(Stub(False))
    finally:
        M.set_lpips(None)
