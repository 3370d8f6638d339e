"""LPIPS on the device (evd_lpips: k_lpips_conv, k_lpips_pool, k_lpips_dist, k_lpips_finish; metrics.LPIPS) against golden G38 -- the
reference's real LPIPS class on the CPU in float32 and in .double(), tools/gen_golden.py G38_lpips -- and, for shapes the fixture does not
hold, against the float64 restatement tests/lpips_ref.py (held to G38's float64 values at 1e-10 by tests/test_lpips_ref.py).

Bound: the relative error against float64 stays within 4 x the largest float32 error of the reference itself that the fixture records over
its cases (ref_f32_err; the project's usual factor, tests/test_gpu_rigid_blur.py) -- the totals against the largest error of a total
(3.9e-7, so 1.6e-6), the per-layer terms against the largest error of a term (3.4e-6, so 1.4e-5).  The device sums a convolution in another
order than the CPU's blocked convolution, so the two float32 results are two samples of the same rounding noise.  The measured errors are
printed per case (profiles/lpips_parity.txt keeps one run's)."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from conftest import load_golden
from evdeblurnerf_amd import metrics as M
from evdeblurnerf_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("G38_lpips")
CASES = [str(c) for c in G["cases"]]
BOUND_VALUE = 4.0 * max(float(G[c + ".ref_f32_err.value"].max()) for c in CASES)
BOUND_TERMS = 4.0 * max(float(G[c + ".ref_f32_err.terms"].max()) for c in CASES)
BACKBONE = W.make_lpips_alexnet_state_dict(int(G["backbone_seed"]))
LINS = [G[f"lin{l}"] for l in range(5)]
HEADS = {f"lin{l}.model.1.weight": LINS[l].reshape(1, -1, 1, 1) for l in range(5)}


def T(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def N(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def model():
    return M.LPIPS(BACKBONE, HEADS)


_REF = {}


def ref(key, pred, target):
    """the float64 yardstick of one input, computed once and shared (read-only)"""
    if key not in _REF:
        _REF[key] = R.lpips(pred, target, BACKBONE, LINS, G["shift"], G["scale"])
    return _REF[key]


def check(tag, value, terms, value64, terms64):
    ev = np.abs(value - value64) / value64
    et = np.abs(terms - terms64) / terms64
    print(f"{tag}: device vs float64: value {ev.max():.2e} (bound {BOUND_VALUE:.2e}), terms {et.max():.2e} (bound {BOUND_TERMS:.2e})")
    assert ev.max() <= BOUND_VALUE, (tag, ev)
    assert et.max() <= BOUND_TERMS, (tag, et)


def test_scaling_constants_are_the_references():
    assert np.array_equal(np.float32(M.LPIPS.SHIFT), G["shift"]) and np.array_equal(np.float32(M.LPIPS.SCALE), G["scale"])


@pytest.mark.parametrize("case", CASES)
def test_g38(model, case):
    B, H, Wd, seed = (int(v) for v in G[case + ".args"])
    pred, target = W.synthetic_frame_pairs(seed, B, H, Wd, *(float(v) for v in G[case + ".range"]))
    value, terms = model(T(pred), T(target), retPerLayer=True)
    assert value.dtype == torch.float64 and value.shape == (B,) and terms.shape == (B, 5) and value.is_cuda
    print(f"{case}: reference float32 vs float64: value {G[case + '.ref_f32_err.value'].max():.2e}, terms {G[case + '.ref_f32_err.terms'].max():.2e}")
    check(case, N(value), N(terms), G[case + ".f64.value"], G[case + ".f64.terms"])
    assert np.allclose(N(terms).sum(axis=1), N(value), rtol=1e-14, atol=0)


# the minimum in each axis alone; three different images, M no multiple of any tile edge (batch strides)
@pytest.mark.parametrize("B,H,Wd", [(1, 31, 64), (1, 64, 31), (3, 95, 131)])
def test_shapes_outside_the_fixture(model, B, H, Wd):
    pred, target = W.synthetic_frame_pairs(3900 + H, B, H, Wd)
    v64, t64 = ref((B, H, Wd), pred, target)
    assert len(set(np.round(v64, 8))) == B                       # every image differs
    value, terms = model(T(pred), T(target), retPerLayer=True)
    check(f"{B} x {H} x {Wd}", N(value), N(terms), v64, t64)


def test_identical_frame_gives_exactly_zero(model):
    pred, target = W.synthetic_frame_pairs(3950, 3, 40, 45)
    target[1] = pred[1]
    v64, t64 = ref("identical", pred, target)
    value, terms = (N(x) for x in model(T(pred), T(target), retPerLayer=True))
    assert value[1] == 0.0 and np.array_equal(terms[1], np.zeros(5))
    assert v64[1] == 0.0
    keep = [0, 2]
    check("identical frame 1", value[keep], terms[keep], v64[keep], t64[keep])


def test_all_features_zero_gives_zero_not_nan():
    dead = {k: (np.full_like(v, -10.0) if k.endswith("bias") else v) for k, v in BACKBONE.items()}
    pred, target = W.synthetic_frame_pairs(3960, 2, 35, 47)
    value, terms = M.LPIPS(dead, HEADS)(T(pred), T(target), retPerLayer=True)
    assert np.array_equal(N(value), np.zeros(2)) and np.array_equal(N(terms), np.zeros((2, 5)))


def test_layouts_and_compute_img_metric(model):
    pred, target = (T(x) for x in W.synthetic_frame_pairs(3970, 2, 33, 41))
    value = model(pred, target)
    assert torch.equal(model(pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)), value)           # [B, 3, H, W]
    assert torch.equal(model(pred, target, format="BHWC"), value)
    assert torch.equal(model(pred[0], target[0]), value[:1])                                            # [H, W, 3]
    assert torch.equal(model(pred[0].permute(2, 0, 1), target[0].permute(2, 0, 1), format="CHW"), value[:1])
    assert torch.equal(model(pred[1].permute(2, 0, 1), target[1].permute(2, 0, 1)), value[1:])         # [3, H, W]
    mean = float((value[0] + value[1]) / 2)
    try:
        M.set_lpips(model)
        got = M.compute_img_metric(pred, target, "lpips")
        assert isinstance(got, float) and got == mean
        mask = torch.zeros((2, 33, 41))
        mask[:, 5:20, 5:30] = 1
        assert M.compute_img_metric(pred, target, "lpips", margin=0.1, mask=mask) == got              # ignored, as in the reference's branch
        assert M.compute_img_metric(pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2), "lpips") == got
    finally:
        M.set_lpips(None)
    with pytest.raises(NotImplementedError, match="weights"):
        M.compute_img_metric(pred, target, "lpips")


def test_bit_equal_and_undisturbed_by_other_calls(model):
    pred, target = (T(x) for x in W.synthetic_frame_pairs(3980, 2, 47, 35))
    other_p, other_t = (T(x) for x in W.synthetic_frame_pairs(3981, 3, 31, 52))
    a_v, a_t = (x.clone() for x in model(pred, target, retPerLayer=True))
    b_v, b_t = (x.clone() for x in model(pred, target, retPerLayer=True))
    assert torch.equal(a_v, b_v) and torch.equal(a_t, b_t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o_v = model(other_p, other_t).clone()
    torch.cuda.current_stream().wait_stream(side)
    c_v, c_t = model(pred, target, retPerLayer=True)
    assert torch.equal(a_v, c_v) and torch.equal(a_t, c_t)
    assert torch.equal(o_v, model(other_p, other_t))             # and an image's value does not depend on the batch it came in
    assert torch.equal(model(other_p[1:2], other_t[1:2]), o_v[1:2])
