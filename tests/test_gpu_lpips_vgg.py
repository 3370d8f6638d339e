"""LPIPS beyond the reference's default call on the device (evd_lpips_create_net, evd_lpips, evd_lpips_spatial; metrics.LPIPS with net, version,
lpips and spatial): the VGG-16 backbone, the spatial map, the baseline without heads and version 0.0, against golden G43 -- the
reference's real LPIPS class with net='vgg' on the CPU in float32 and in .double(), tools/gen_golden.py G43_lpips_vgg -- and, for shapes
and for the AlexNet options the fixture does not hold, against the float64 restatement tests/lpips_vgg_ref.py (held to G43's float64 arrays
at 1e-10 by tests/test_lpips_vgg_ref.py).

Bounds: the error against float64 stays within 4 x the largest float32 error of the reference itself that G43 records over its cases
(ref_f32_err; the project's usual factor, tests/test_gpu_lpips.py), separately for the totals, the per-layer terms and the maps, and
separately for the heads and the baseline.  Values and terms are relative errors; a map's error is its largest absolute error over the
largest value of the float64 map, per image (per image and layer for the per-layer maps, which are held to the same bound as the map).
Version 0.0 and the AlexNet maps, of which the fixture has no error record of their own over several cases, use the bound of the VGG
heads.  The device sums a convolution in another order than the CPU, so the two float32 results are two samples of the same rounding
noise.  The measured errors are printed per case (profiles/lpips_vgg_parity.txt keeps one run's)."""
import numpy as np
import pytest
import torch

import lpips_vgg_ref as RV
from conftest import load_golden
from evdeblurnerf_amd import _lib
from evdeblurnerf_amd import metrics as M
from evdeblurnerf_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("G43_lpips_vgg")
G38 = load_golden("G38_lpips")
CASES = [str(c) for c in G["cases"]]
V00 = str(G["v00_case"])
BOUND = {(kind, pre): 4.0 * max(float(G[f"{c}.{pre}ref_f32_err.{kind}"].max()) for c in CASES)
         for kind in ("value", "terms", "map") for pre in ("", "base.")}
BACKBONE = {"vgg": W.make_lpips_vgg16_state_dict(int(G["backbone_seed"])), "alex": W.make_lpips_alexnet_state_dict(int(G38["backbone_seed"]))}
LINS = {"vgg": [G[f"lin{l}"] for l in range(5)], "alex": [G38[f"lin{l}"] for l in range(5)]}
HEADS = {net: {f"lin{l}.model.1.weight": LINS[net][l].reshape(1, -1, 1, 1) for l in range(5)} for net in LINS}
ZERO, ONE = np.zeros(3, np.float32), np.ones(3, np.float32)


def T(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def N(x):
    return x.detach().cpu().numpy()


_MODELS = {}


def model(net="vgg", lpips=True, spatial=False, version="0.1"):
    """one model per configuration, built once"""
    key = (net, lpips, spatial, version)
    if key not in _MODELS:
        _MODELS[key] = M.LPIPS(BACKBONE[net], HEADS[net] if lpips else None, net=net, version=version, lpips=lpips, spatial=spatial)
    return _MODELS[key]


_REF = {}


def ref(key, pred, target, net="vgg", lpips=True):
    """the float64 yardstick of one input, computed once and shared (read-only): value, terms, map, layer maps"""
    key = (key, net, lpips)
    if key not in _REF:
        args = (pred, target, BACKBONE[net], LINS[net] if lpips else None, G["shift"], G["scale"])
        _REF[key] = RV.lpips(*args, net=net) + RV.lpips_spatial(*args, net=net)
    return _REF[key]


def case_inputs(case):
    B, H, Wd, seed = (int(v) for v in G[case + ".args"])
    return W.synthetic_frame_pairs(seed, B, H, Wd, *(float(v) for v in G[case + ".range"]))


def check(tag, value, terms, value64, terms64, pre=""):
    ev = np.abs(value - value64) / value64
    et = np.abs(terms - terms64) / terms64
    bv, bt = BOUND["value", pre], BOUND["terms", pre]
    print(f"{tag}: device vs float64: value {ev.max():.2e} (bound {bv:.2e}), terms {et.max():.2e} (bound {bt:.2e})")
    assert ev.max() <= bv, (tag, ev)
    assert et.max() <= bt, (tag, et)


def map_err(got, want):
    return np.abs(got - want).max(axis=(-2, -1)) / np.abs(want).max(axis=(-2, -1))


def check_maps(tag, smap, layers, map64, layers64, pre=""):
    B, _, H, Wd = smap.shape
    assert smap.dtype == torch.float32 and smap.is_cuda and layers.dtype == torch.float32 and layers.shape == (B, 5, H, Wd)
    em = map_err(N(smap)[:, 0].astype(np.float64), map64)
    el = map_err(N(layers).astype(np.float64), layers64)
    b = BOUND["map", pre]
    print(f"{tag}: device vs float64: map {em.max():.2e}, layer maps {el.max():.2e} (bound {b:.2e})")
    assert em.max() <= b, (tag, em)
    assert el.max() <= b, (tag, el)


def test_new_keywords_exist():
    """the constructor of the feature: fails on a library without it"""
    assert model().net == "vgg" and not model().spatial and model(spatial=True).spatial
    assert M.LPIPS(BACKBONE["vgg"], HEADS["vgg"], net="vgg16").net == "vgg"


@pytest.mark.parametrize("case", CASES)
def test_g43(case):
    pred, target = case_inputs(case)
    B = pred.shape[0]
    value, terms = model()(T(pred), T(target), retPerLayer=True)
    assert value.dtype == torch.float64 and value.shape == (B,) and terms.shape == (B, 5) and value.is_cuda
    print(f"{case}: reference float32 vs float64: value {G[case + '.ref_f32_err.value'].max():.2e}, terms {G[case + '.ref_f32_err.terms'].max():.2e}")
    check(case, N(value), N(terms), G[case + ".f64.value"], G[case + ".f64.terms"])
    assert np.allclose(N(terms).sum(axis=1), N(value), rtol=1e-14, atol=0)


# the minimum in each axis with an odd other side; three different images, floor pools inexact at every level, M no multiple of the tile
@pytest.mark.parametrize("B,H,Wd", [(1, 16, 17), (1, 17, 16), (3, 35, 53)])
def test_shapes_outside_the_fixture(B, H, Wd):
    pred, target = W.synthetic_frame_pairs(4350 + H, B, H, Wd)
    v64, t64, m64, l64 = ref((B, H, Wd), pred, target)
    assert len(set(np.round(v64, 8))) == B                       # every image differs
    value, terms = model()(T(pred), T(target), retPerLayer=True)
    check(f"{B} x {H} x {Wd}", N(value), N(terms), v64, t64)
    smap, layers = model(spatial=True)(T(pred), T(target), retPerLayer=True)
    check_maps(f"{B} x {H} x {Wd}", smap, layers, m64, l64)


@pytest.mark.parametrize("pre", ["", "base."])
@pytest.mark.parametrize("case", CASES)
def test_g43_spatial_map(case, pre):
    """heads and baseline: the map against the fixture, the per-layer maps against the fixture where it keeps them, else the restatement"""
    pred, target = case_inputs(case)
    B, H, Wd = pred.shape[:3]
    k = f"{case}.{pre}"
    l64 = G[k + "f64.layer_maps"] if k + "f64.layer_maps" in G else ref(case, pred, target, lpips=not pre)[3]
    m = model(lpips=not pre, spatial=True)
    smap, layers = m(T(pred), T(target), retPerLayer=True)
    assert smap.shape == (B, 1, H, Wd)
    print(f"{k[:-1]}: reference float32 vs float64: map {G[k + 'ref_f32_err.map'].max():.2e}, layer maps {G[k + 'ref_f32_err.layer_maps'].max():.2e}")
    check_maps(k[:-1], smap, layers, G[k + "f64.map"], l64, pre)
    assert torch.equal(m(T(pred), T(target)), smap)              # without retPerLayer: the same map


@pytest.mark.parametrize("case", CASES)
def test_g43_baseline(case):
    pred, target = case_inputs(case)
    value, terms = model(lpips=False)(T(pred), T(target), retPerLayer=True)
    k = case + ".base."
    check(k[:-1], N(value), N(terms), G[k + "f64.value"], G[k + "f64.terms"], "base.")
    assert np.allclose(N(terms).sum(axis=1), N(value), rtol=1e-14, atol=0)


def test_g43_version_0_0():
    pred, target = case_inputs(V00)
    k = V00 + ".v00."
    value, terms = model(version="0.0")(T(pred), T(target), retPerLayer=True)
    check(k[:-1], N(value), N(terms), G[k + "f64.value"], G[k + "f64.terms"])
    smap, layers = model(version="0.0", spatial=True)(T(pred), T(target), retPerLayer=True)
    check_maps(k[:-1], smap, layers, G[k + "f64.map"], G[k + "f64.layer_maps"])
    assert not np.allclose(N(value), G[V00 + ".f64.value"], rtol=1e-3)      # and it is not version 0.1


# AlexNet: stride 4 and two 3 x 3 pools, so every map is resampled; the second shape has 1 x 1 maps after the second pool in one axis
@pytest.mark.parametrize("lpips", [True, False])
@pytest.mark.parametrize("B,H,Wd", [(2, 35, 47), (1, 31, 40)])
def test_alexnet_spatial_map_and_baseline(B, H, Wd, lpips):
    pred, target = W.synthetic_frame_pairs(4360 + H, B, H, Wd)
    v64, t64, m64, l64 = ref(("alex", B, H, Wd), pred, target, net="alex", lpips=lpips)
    pre = "" if lpips else "base."
    tag = f"alex {pre}{B} x {H} x {Wd}"
    smap, layers = model("alex", lpips=lpips, spatial=True)(T(pred), T(target), retPerLayer=True)
    assert smap.shape == (B, 1, H, Wd)
    check_maps(tag, smap, layers, m64, l64, pre)
    if not lpips:                                                # (with heads: tests/test_gpu_lpips.py)
        value, terms = model("alex", lpips=False)(T(pred), T(target), retPerLayer=True)
        check(tag, N(value), N(terms), v64, t64, "base.")


def test_identical_frame_gives_exactly_zero():
    pred, target = W.synthetic_frame_pairs(4370, 3, 33, 37)
    target[1] = pred[1]
    v64, t64, m64, l64 = ref("identical", pred, target)
    assert v64[1] == 0.0 and not m64[1].any()
    value, terms = (N(x) for x in model()(T(pred), T(target), retPerLayer=True))
    smap, layers = model(spatial=True)(T(pred), T(target), retPerLayer=True)
    assert value[1] == 0.0 and np.array_equal(terms[1], np.zeros(5))
    assert not N(smap)[1].any() and not N(layers)[1].any()
    keep = [0, 2]
    check("identical frame 1", value[keep], terms[keep], v64[keep], t64[keep])
    check_maps("identical frame 1", smap[keep], layers[keep], m64[keep], l64[keep])
    amap = model("alex", spatial=True)(T(np.tile(pred, (1, 2, 1, 1))), T(np.tile(target, (1, 2, 1, 1))))
    assert not N(amap)[1].any() and N(amap)[0].any()


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_all_features_zero_gives_zero_not_nan(net):
    dead = {k: (np.full_like(v, -10.0) if k.endswith("bias") else v) for k, v in BACKBONE[net].items()}
    pred, target = W.synthetic_frame_pairs(4380, 2, 35, 47)
    value, terms = M.LPIPS(dead, HEADS[net], net=net)(T(pred), T(target), retPerLayer=True)
    assert np.array_equal(N(value), np.zeros(2)) and np.array_equal(N(terms), np.zeros((2, 5)))
    smap, layers = M.LPIPS(dead, None, net=net, lpips=False, spatial=True)(T(pred), T(target), retPerLayer=True)
    assert np.array_equal(N(smap), np.zeros((2, 1, 35, 47), np.float32)) and np.array_equal(N(layers), np.zeros((2, 5, 35, 47), np.float32))


def test_layouts_and_compute_img_metric():
    pred, target = (T(x) for x in W.synthetic_frame_pairs(4390, 2, 19, 30))
    for m in (model(), model(spatial=True)):
        value = m(pred, target)
        assert torch.equal(m(pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)), value)               # [B, 3, H, W]
        assert torch.equal(m(pred, target, format="BHWC"), value)
        assert torch.equal(m(pred[0], target[0]), value[:1])                                            # [H, W, 3]
        assert torch.equal(m(pred[0].permute(2, 0, 1), target[0].permute(2, 0, 1), format="CHW"), value[:1])
    value = model()(pred, target)
    mean = float((value[0] + value[1]) / 2)
    assert float(model().mean(pred, target)) == mean
    try:
        M.set_lpips(model())
        got = M.compute_img_metric(pred, target, "lpips")
        assert isinstance(got, float) and got == mean
        assert M.compute_img_metric(pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2), "lpips") == got
        with pytest.raises(_lib.EvdError, match="spatial"):
            M.set_lpips(model(spatial=True))
        assert M.compute_img_metric(pred, target, "lpips") == got                                       # the refused model replaced nothing
    finally:
        M.set_lpips(None)
    with pytest.raises(_lib.EvdError, match="spatial"):
        model(spatial=True).mean(pred, target)
    with pytest.raises(_lib.EvdError, match="vgg16.*at least 16"):
        model()(pred[:, :15], target[:, :15])


def test_bit_equal_and_undisturbed_by_other_calls():
    pred, target = (T(x) for x in W.synthetic_frame_pairs(4391, 2, 29, 35))
    other_p, other_t = (T(x) for x in W.synthetic_frame_pairs(4392, 3, 31, 52))
    vgg, vmap, alex = model(), model(spatial=True), model("alex")
    a_v, a_t = (x.clone() for x in alex(other_p, other_t, retPerLayer=True))
    v_v, v_t = (x.clone() for x in vgg(pred, target, retPerLayer=True))
    m_v, m_l = (x.clone() for x in vmap(pred, target, retPerLayer=True))
    w_v, w_t = vgg(pred, target, retPerLayer=True)
    n_v, n_l = vmap(pred, target, retPerLayer=True)
    assert torch.equal(v_v, w_v) and torch.equal(v_t, w_t) and torch.equal(m_v, n_v) and torch.equal(m_l, n_l)     # two calls
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    b_v = alex(other_p, other_t).clone()
    with torch.cuda.stream(side):                                # a VGG call on a side stream between two AlexNet calls
        s_v = vgg(pred, target).clone()
        s_m = vmap(pred, target).clone()
    c_v, c_t = alex(other_p, other_t, retPerLayer=True)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a_v, b_v) and torch.equal(a_v, c_v) and torch.equal(a_t, c_t)
    assert torch.equal(s_v, v_v) and torch.equal(s_m, m_v)
    assert torch.equal(vgg(pred[1:2], target[1:2]), v_v[1:2])   # an image alone equals the same image inside a batch
    assert torch.equal(vmap(pred[1:2], target[1:2]), m_v[1:2])
    am = model("alex", spatial=True)
    assert torch.equal(am(other_p[2:3], other_t[2:3]), am(other_p, other_t)[2:3])


def test_alexnet_is_untouched():
    """net='alex' through the keywords is the positional form, bit for bit, on a G38 case"""
    B, H, Wd, seed = (int(v) for v in G38["odd.args"])
    pred, target = (T(x) for x in W.synthetic_frame_pairs(seed, B, H, Wd))
    old = M.LPIPS(BACKBONE["alex"], HEADS["alex"])
    new = M.LPIPS(BACKBONE["alex"], lin=HEADS["alex"], net="alex", version="0.1", lpips=True, spatial=False)
    o_v, o_t = old(pred, target, retPerLayer=True)
    n_v, n_t = new(pred, target, retPerLayer=True)
    assert torch.equal(o_v, n_v) and torch.equal(o_t, n_t) and torch.equal(old.mean(pred, target), new.mean(pred, target))
    ev = np.abs(N(o_v) - G38["odd.f64.value"]) / G38["odd.f64.value"]
    assert ev.max() <= 4.0 * max(float(G38[str(c) + ".ref_f32_err.value"].max()) for c in G38["cases"])
