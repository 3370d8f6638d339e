"""CPU-only.  (1) The float64 restatement tests/img_metric_ref.py of the reference's compute_img_metric, the yardstick of
tests/test_gpu_img_metrics.py, against facts that do not depend on it: closed forms, and an explicit padded-array computation of the
reflect border.  scikit-image is not installed here, so the reference's own function cannot be run to make a golden; the restatement is
written from scikit-image 0.19.2's algorithm on top of scipy.ndimage.uniform_filter, the function scikit-image itself calls.
(2) What the reference's own float32 arithmetic loses against float64, printed per shape.  Recorded from this test (mean SSIM, |float32 mode
- float64 mode|, two smooth images + noise 0.002): 7 x 7: 1.5e-07, 9 x 13: 3.2e-08, 17 x 33: 4.2e-08, 41 x 70: 2.0e-08; without the noise
1.3e-07, 3.2e-08, 3.9e-08, 2.5e-08 (the variance uxx - ux ux cancels against C2 = 3.6e-3); MSE 2e-13 .. 8e-12, PSNR 5e-10 .. 2e-08 dB.  The
device kernel accumulates in float64 and is held to 1e-9 in SSIM.
(3) The new C entries reject bad arguments before they touch the device."""
import ctypes as C

import numpy as np
import pytest

import img_metric_ref as R


def const_pair(a, b, h=9, w=11):
    """images whose MAPPED values are the constants a and b"""
    return np.full((1, h, w, 3), (a + 1) / 2, np.float32), np.full((1, h, w, 3), (b + 1) / 2, np.float32)


@pytest.mark.parametrize("a,b", [(0.5, 0.25), (-0.75, 0.5), (0.0, 1.0), (-1.0, 1.0), (0.125, 0.125)])
def test_constant_images_closed_form(a, b):
    """constant images: every variance is 0, so S = (2ab + C1) / (a^2 + b^2 + C1) everywhere; mse = (a - b)^2"""
    p, t = const_pair(a, b)
    r = R.img_metrics_ref(p, t)
    want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert abs(r["ssim"][0] - want) < 1e-14 and abs(r["mse"][0] - (a - b) ** 2) < 1e-15
    m = np.ones((1, 9, 11, 1), np.float32)
    assert abs(R.img_metrics_ref(p, t, mask=m)["ssim"][0] - want) < 1e-14           # the whole region, reflect border: still constant


def test_identical_images():
    p, _ = R.smooth_images(1, 2, 12, 15)
    r = R.img_metrics_ref(p, p)
    assert np.all(r["ssim"] == 1.0) and np.all(r["mse"] == 0.0) and np.all(np.isposinf(r["psnr"]))


def test_psnr_data_range_switch():
    """a prediction with every pixel >= 0.5 (mapped >= 0: data_range 1) and one with a single pixel below (data_range 2) differ by
    20 log10 2 dB at equal MSE"""
    rs = np.random.RandomState(2)
    p = rs.uniform(0.5, 1.0, (1, 8, 10, 3)).astype(np.float32)
    t = p.copy()
    d = np.float32(0.125)
    p[0, 4, 4, 1] = 0.5 + d                   # mapped +0.25 against a target of mapped 0
    t[0, 4, 4, 1] = 0.5
    q, u = p.copy(), t.copy()
    q[0, 4, 4, 1] = 0.5 - d                   # mapped -0.25: the same squared difference, one negative value
    a, b = R.img_metrics_ref(p, t), R.img_metrics_ref(q, u)
    assert a["mse"][0] == b["mse"][0] > 0
    assert abs((b["psnr"][0] - a["psnr"][0]) - 20 * np.log10(2)) < 1e-12
    assert abs(a["psnr"][0] - 10 * np.log10(1.0 / a["mse"][0])) < 1e-12


def test_mask_correction_and_zero_pixels_count_toward_the_minimum():
    rs = np.random.RandomState(3)
    p = rs.uniform(0.6, 1.0, (1, 8, 10, 3)).astype(np.float32)      # mapped > 0 everywhere: data_range 1 with or without a mask of zeros
    t = rs.uniform(0.6, 1.0, (1, 8, 10, 3)).astype(np.float32)
    m = (rs.rand(1, 8, 10, 1) < 0.5).astype(np.float32)
    r = R.img_metrics_ref(p, t, mask=m)
    x, y = R.to_range(p).astype(np.float64), R.to_range(t).astype(np.float64)
    mse = ((x - y) ** 2 * m).sum() / (8 * 10 * 3)
    corr = 10 * np.log10(80 / m.sum(dtype=np.float64))
    assert abs(r["mse"][0] - (mse - corr)) < 1e-13 and abs(r["psnr"][0] - (10 * np.log10(1 / mse) - corr)) < 1e-11


@pytest.mark.parametrize("h,w", [(7, 7), (8, 12), (11, 9)])
def test_reflect_border_against_explicit_padding(h, w):
    """S on the whole region with uniform_filter's default border = the same window means on an explicitly padded array
    (np.pad mode 'symmetric' is scipy's 'reflect': d c b a | a b c d | d c b a), summed window by window"""
    p, t = R.smooth_images(10 + h, 1, h, w)
    x, y = R.to_range(p)[0, ..., 1].astype(np.float64), R.to_range(t)[0, ..., 1].astype(np.float64)
    S = R.ssim_map(x, y)
    xp, yp = np.pad(x, 3, mode="symmetric"), np.pad(y, 3, mode="symmetric")
    cn = 49 / 48
    want = np.empty_like(S)
    for i in range(h):
        for j in range(w):
            a, b = xp[i:i + 7, j:j + 7], yp[i:i + 7, j:j + 7]
            ux, uy = a.mean(), b.mean()
            vx, vy, vxy = cn * ((a * a).mean() - ux * ux), cn * ((b * b).mean() - uy * uy), cn * ((a * b).mean() - ux * uy)
            want[i, j] = (2 * ux * uy + R.C1) * (2 * vxy + R.C2) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))
    assert np.abs(S - want).max() < 1e-11
    assert xp[0, 3] == x[2, 0] and xp[2, 3] == x[0, 0] and xp[-1, 3] == x[-3, 0]    # half-sample symmetric, not 'mirror'


def test_region_smaller_than_the_window_raises():
    p, t = R.smooth_images(4, 1, 6, 9)
    with pytest.raises(ValueError):
        R.img_metrics_ref(p, t)
    p, t = R.smooth_images(4, 1, 20, 27)
    assert R.margins(20, 27, 0.1) == (3, 3) and R.margins(20, 27, 0) == (0, 0)
    with pytest.raises(ValueError):
        R.img_metrics_ref(p, t, margin=0.3)           # 20 - 2 * 7 = 6 rows


def test_float32_mode_against_float64_mode():
    """what scikit-image 0.19.2's float32 arithmetic loses: u32 = 6e-8 on uxx, ux ux <= 1, divided by C2 = 3.6e-3, is at most ~2e-5 per
    pixel of S and far less in the mean; the figures are printed (and recorded in this file's docstring), the assertion is that bound"""
    for noise in (0.002, 0.0):
        for h, w in ((7, 7), (9, 13), (17, 33), (41, 70)):
            p, t = R.smooth_images(100 + h, 2, h, w, noise=noise, overshoot=False)
            r64, r32 = R.img_metrics_ref(p, t), R.img_metrics_ref(p, t, dtype=np.float32)
            gap = {k: float(np.abs(r64[k] - r32[k]).max()) for k in r64}
            print(f"noise {noise}: {h} x {w}: |float32 mode - float64 mode| ssim {gap['ssim']:.1e} mse {gap['mse']:.1e} psnr {gap['psnr']:.1e} dB")
            assert gap["ssim"] < 2e-5 and gap["mse"] < 1e-7 and gap["psnr"] < 1e-4


@pytest.fixture(scope="module")
def lib():
    from evdeblurnerf_amd import build, _lib
    build.build()
    return _lib.lib()


def metrics_call(h, B=1, H=9, W=13, mh=0, mw=0, mask=0, mask_ch=1, pred=1, target=1, out=1, ws=1, ws_bytes=None):
    """pointers are dummies (non-null = 0x1000): a valid call is never made here"""
    P = lambda on: C.c_void_p(0x1000) if on else None
    need = h.evd_img_metrics_workspace_bytes(max(B, 1), max(H, 7), max(W, 7))
    return h.evd_img_metrics(P(pred), P(target), P(mask), mask_ch, B, H, W, mh, mw, P(out), P(ws), need if ws_bytes is None else ws_bytes, None)


def test_entries_reject_bad_arguments_without_a_gpu(lib):
    for kw in ({"H": 6}, {"W": 6}, {"H": 20, "W": 27, "mh": 7, "mw": 3}, {"H": 20, "W": 27, "mh": 3, "mw": 11}, {"B": 0}, {"H": 0}, {"mh": -1},
               {"mask": 1, "mask_ch": 2}, {"pred": 0}, {"target": 0}, {"out": 0}, {"ws": 0}, {"ws_bytes": 39}):
        assert metrics_call(lib, **kw) == -1, kw
        assert b"evd_img_metrics" in lib.evd_last_error(), kw
    assert metrics_call(lib, H=6) == -1 and b"7 x 7" in lib.evd_last_error()
    assert lib.evd_to8b(None, 5, C.c_void_p(0x1000), None) == -1 and b"evd_to8b" in lib.evd_last_error()
    assert lib.evd_to8b(C.c_void_p(0x1000), -1, C.c_void_p(0x1000), None) == -1
    assert lib.evd_to8b(None, 0, None, None) == 0                                    # nothing to do: no launch


def test_workspace_bytes(lib):
    from evdeblurnerf_amd import metrics as M
    f = lib.evd_img_metrics_workspace_bytes
    for bad in ((0, 9, 9), (1, 6, 9), (1, 9, 6)):
        assert f(*bad) == 0, bad
    th, tw = M.TILE_H, M.TILE_W
    assert f(1, th, tw) >= 40 and f(1, th + 1, tw + 1) >= 4 * 40 and f(3, 2 * th - 1, 2 * tw - 1) >= 3 * 4 * 40
    assert f(8, 400, 400) < 1 << 20 and f(2, 400, 400) > f(1, 400, 400)


def test_tile_constants_agree_with_the_header():
    import os
    import re
    from conftest import ROOT
    from evdeblurnerf_amd import metrics as M
    src = open(os.path.join(ROOT, "include", "evdnerf.h")).read()
    d = dict(re.findall(r"#define EVD_IMG_METRICS_TILE_([HW]) (\d+)", src))
    assert (int(d["H"]), int(d["W"])) == (M.TILE_H, M.TILE_W)


def test_lpips_and_unknown_metric():
    from evdeblurnerf_amd import metrics as M
    with pytest.raises(NotImplementedError, match="weights"):
        M.compute_img_metric(None, None, "lpips")
    with pytest.raises(RuntimeError, match="not recognized"):
        M.compute_img_metric(None, None, "l1")
