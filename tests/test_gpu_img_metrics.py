"""Image metrics on the device (evd_img_metrics: k_img_metrics, k_img_metrics_finish; evd_to8b) against the float64 restatement
tests/img_metric_ref.py of the reference's compute_img_metric (scikit-image is not installed here, so the reference's own function cannot
be run to make a golden; tests/test_img_metric_ref.py checks the restatement against closed forms).

Tolerances: SSIM 1e-9 absolute, MSE 1e-10 relative, PSNR 1e-9 dB absolute.  Derived, not measured: the inputs are float32 values whose
products are exact in float64; sums of at most 49 terms and of the pixel count round at 2^-53 per step; the SSIM quotient amplifies by at most
1 / C1 + 1 / C2 ~ 2.8e3; that puts the error near 1e-11 and the allowance adds two orders.  The worst observed ratio to the tolerance is
printed per case."""
import numpy as np
import pytest
import torch

import img_metric_ref as R
from evdeblurnerf_amd.metrics import TILE_H, TILE_W

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"ssim": 1e-9, "mse": 1e-10, "psnr": 1e-9}


def T(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def N(x):
    return x.detach().cpu().numpy()


# (B, H, W, margin): one valid window; three different images; one more than the kernel's tile and one less than twice the tile in each
# dimension; a window that starts at row 3, column 3 of the frame
SHAPES = [(1, 7, 7, 0), (3, 9, 13, 0), (2, TILE_H + 1, TILE_W + 1, 0), (2, 2 * TILE_H - 1, 2 * TILE_W - 1, 0), (2, 20, 27, 0.1)]


_CASES = {}


def case(B, H, W, margin, mask_ch=0):
    """inputs and the float64 reference of one case, computed once and shared (read-only)"""
    key = (B, H, W, margin, mask_ch)
    if key not in _CASES:
        pred, target = R.smooth_images(3700 + 31 * H + W, B, H, W)
        mask = None
        if mask_ch:                                      # the same binary mask for the whole batch: the reference and the per-image rule coincide
            rs = np.random.RandomState(3750 + mask_ch)
            mask = np.broadcast_to((rs.rand(1, H, W, mask_ch) < 0.7).astype(np.float32), (B, H, W, mask_ch)).copy()
        ref = R.img_metrics_ref(pred, target, margin=margin, mask=mask)
        for v in (pred, target, mask, *ref.values()):
            if v is not None:
                v.setflags(write=False)
        _CASES[key] = (pred, target, mask, ref)
    return _CASES[key]


def check(got, ref, label):
    worst = {}
    for k in ("mse", "psnr", "ssim"):
        g = N(got[k])
        assert g.dtype == np.float64 and g.shape == ref[k].shape
        scale = np.abs(ref[k]) if k == "mse" else 1.0
        err = np.abs(g - ref[k]) / scale
        worst[k] = float(err.max() / TOL[k])
        print(f"{label}: {k} {g} worst err / tolerance {worst[k]:.3e}")
    for k in ("mse", "psnr", "ssim"):
        assert worst[k] <= 1.0, (label, k, worst[k])
        m = float(got[k + "_mean"])
        want = float(np.mean(ref[k]))
        assert abs(m - want) <= TOL[k] * (abs(want) if k == "mse" else 1.0), (label, k + "_mean")
    assert np.all((ref["ssim"] > 0.05) & (ref["ssim"] < 0.98)), ref["ssim"]       # well inside (0, 1)


@pytest.mark.parametrize("B,H,W,margin", SHAPES)
def test_against_the_restatement(B, H, W, margin):
    from evdeblurnerf_amd.metrics import img_metrics
    pred, target, _, ref = case(B, H, W, margin)
    assert pred.min() < 0 and pred.max() > 1                                       # the clamp is exercised
    got = img_metrics(T(pred), T(target), margin=margin)
    check(got, ref, f"{B} x {H} x {W} margin {margin}")
    again = img_metrics(T(pred), T(target), margin=margin)                         # the same call twice: equal bits
    for k in got:
        assert torch.equal(got[k], again[k]), k
    for i in range(B):                                                             # an image alone: the same bits as inside its batch
        one = img_metrics(T(pred[i:i + 1]), T(target[i:i + 1]), margin=margin)
        for k in ("mse", "psnr", "ssim"):
            assert torch.equal(one[k][0], got[k][i]), (k, i)


@pytest.mark.parametrize("mask_ch,B,H,W,margin", [(1, 2, 20, 27, 0.1), (3, 1, 2 * TILE_H - 1, 2 * TILE_W - 1, 0)])
def test_masked(mask_ch, B, H, W, margin):
    from evdeblurnerf_amd.metrics import img_metrics
    pred, target, mask, ref = case(B, H, W, margin, mask_ch)
    got = img_metrics(T(pred), T(target), margin=margin, mask=T(mask).permute(0, 3, 1, 2))
    check(got, ref, f"mask Cm {mask_ch}, {B} x {H} x {W} margin {margin}")
    again = img_metrics(T(pred), T(target), margin=margin, mask=T(mask).permute(0, 3, 1, 2))
    for k in got:
        assert torch.equal(got[k], again[k]), k
    if mask_ch == 1:                                                               # [B, H, W] is the same mask
        flat = img_metrics(T(pred), T(target), margin=margin, mask=T(mask[..., 0]))
        for k in got:
            assert torch.equal(got[k], flat[k]), k


def test_compute_img_metric_layouts():
    """the mean of the per-image values, as a Python float, for the three metrics and every accepted layout"""
    from evdeblurnerf_amd.metrics import compute_img_metric, img_metrics
    B, H, W = 3, 9, 13
    pred, target, _, ref = case(B, H, W, 0)
    p, t = T(pred), T(target)
    per = img_metrics(p, t)
    for metric in ("mse", "psnr", "ssim"):
        want = float(np.mean(ref[metric]))
        tol = TOL[metric] * (abs(want) if metric == "mse" else 1.0)
        for fmt, a, b in ((None, p, t), ("BHWC", p, t), (None, p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2)), ("BCHW", p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2))):
            v = compute_img_metric(a, b, metric, format=fmt)
            assert isinstance(v, float) and abs(v - want) <= tol, (metric, fmt, v, want)
            assert v == float(per[metric + "_mean"]) and abs(v - float(N(per[metric]).mean())) <= tol
        for fmt, a, b in ((None, p[1], t[1]), ("HWC", p[1], t[1]), ("CHW", p[1].permute(2, 0, 1), t[1].permute(2, 0, 1))):     # 3-D input
            v = compute_img_metric(a, b, metric, format=fmt)
            assert isinstance(v, float) and v == float(per[metric][1]), (metric, fmt)
    _, _, mask, mref = case(2, 20, 27, 0.1, 1)
    pred, target = case(2, 20, 27, 0.1, 1)[:2]
    for mk in (T(mask[..., 0]), T(mask).permute(0, 3, 1, 2), T(mask).permute(0, 3, 1, 2).expand(-1, 3, -1, -1)):               # [B,H,W], [B,1,H,W], [B,3,H,W]
        v = compute_img_metric(T(pred), T(target), "ssim", margin=0.1, mask=mk)
        assert abs(v - float(np.mean(mref["ssim"]))) <= TOL["ssim"]
    with pytest.raises(NotImplementedError):
        compute_img_metric(p, t, "lpips")
    with pytest.raises(RuntimeError):
        compute_img_metric(p, t, "l2")


def test_special_values():
    """identical images: SSIM 1, MSE 0, PSNR +inf; a prediction without a negative mapped value: data_range 1; NaN in, NaN out; a region
    smaller than the window is rejected"""
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.metrics import img_metrics
    pred, target, _, _ = case(3, 9, 13, 0)
    same = img_metrics(T(target), T(target))
    assert torch.all(same["ssim"] == 1.0) and torch.all(same["mse"] == 0.0) and torch.all(torch.isposinf(same["psnr"]))
    rs = np.random.RandomState(3790)
    p = rs.uniform(0.5, 1.0, (2, 9, 13, 3)).astype(np.float32)
    t = rs.uniform(0.0, 1.0, (2, 9, 13, 3)).astype(np.float32)
    p[1, 4, 5, 2] = 0.25                                                           # image 1 has one negative mapped value: data_range 2
    ref = R.img_metrics_ref(p, t)
    got = img_metrics(T(p), T(t))
    assert np.abs(N(got["psnr"]) - ref["psnr"]).max() <= TOL["psnr"]
    assert abs(ref["psnr"][0] - 10 * np.log10(1.0 / ref["mse"][0])) < 1e-12 and abs(ref["psnr"][1] - 10 * np.log10(4.0 / ref["mse"][1])) < 1e-12
    bad = pred.copy()
    bad[1, 2, 3, 0] = np.nan
    g = img_metrics(T(bad), T(target))
    for k in ("mse", "psnr", "ssim"):
        assert np.array_equal(np.isnan(N(g[k])), [False, True, False]), k
        assert torch.equal(g[k][0], img_metrics(T(pred), T(target))[k][0])
    with pytest.raises(L.EvdError, match="7 x 7"):
        img_metrics(T(pred[:, :6]), T(target[:, :6]))
    with pytest.raises(L.EvdError, match="7 x 7"):
        img_metrics(T(pred), T(target), margin=0.2)                                # int(9 * 0.2) + 1 = 2 rows off each side: 5 left
    ok = img_metrics(T(pred), T(target), margin=0.1)                               # 7 rows, 9 columns
    assert np.abs(N(ok["ssim"]) - R.img_metrics_ref(pred, target, margin=0.1)["ssim"]).max() <= TOL["ssim"]


def test_to8b():
    from evdeblurnerf_amd.metrics import to8b
    k = np.arange(1, 256, dtype=np.float64)
    edges = np.concatenate([np.nextafter((k / 255).astype(np.float32), np.float32(0)), (k / 255).astype(np.float32), np.nextafter((k / 255).astype(np.float32), np.float32(2))])
    rs = np.random.RandomState(3795)
    x = np.concatenate([np.array([0.0, 1.0, -0.0, -1e-8, -3.5, 1.0000001, 7.25, np.inf, -np.inf, 0.999999, 0.5], np.float32), edges,
                        rs.uniform(-0.2, 1.2, 4099).astype(np.float32)])
    want = (255 * np.clip(x, 0, 1)).astype(np.uint8)
    got = to8b(T(x))
    assert got.dtype == torch.uint8 and got.is_cuda and np.array_equal(N(got), want)
    assert {0, 1, 127, 254, 255} <= set(want.tolist())
    for off, n in ((1, 13), (3, 6), (0, 3), (2, 1)):                               # unaligned views, lengths that are no multiple of 4
        assert np.array_equal(N(to8b(T(x)[off:off + n])), want[off:off + n]), (off, n)
    img = rs.uniform(-0.1, 1.1, (2, 5, 7, 3)).astype(np.float32)
    assert np.array_equal(N(to8b(T(img))), (255 * np.clip(img, 0, 1)).astype(np.uint8))
    nan = np.array([0.3, np.nan, 0.9, np.nan, 1.0], np.float32)
    assert N(to8b(T(nan))).tolist() == [76, 0, 229, 0, 255]
    assert to8b(T(x)[:0]).shape == (0,)
