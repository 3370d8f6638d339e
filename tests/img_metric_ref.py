"""Restatement of the reference's compute_img_metric (utils/metrics.py:18-100) for 'mse', 'psnr' and 'ssim', the yardstick of
tests/test_gpu_img_metrics.py.

scikit-image is not installed where this suite runs, so the reference's own function cannot be executed to make a golden.  This file
restates scikit-image 0.19.2 (the version the reference pins): metrics.mean_squared_error, metrics.peak_signal_noise_ratio and
metrics.structural_similarity(multichannel=True, full=True) with the defaults the reference leaves in place (win_size 7, uniform window,
K1 0.01, K2 0.03, use_sample_covariance, data_range 2 for float images), on top of scipy.ndimage.uniform_filter: the function scikit-image
itself calls.  tests/test_img_metric_ref.py checks it against closed forms and an explicit padded-array computation.

`dtype` is the arithmetic after the reference's float32 mapping: np.float64 is the yardstick; np.float32 is what scikit-image 0.19.2 does
with float32 images (the filters, the variances and S stay float32; the means are accumulated in float64).

With a mask every image is multiplied by its own mask (the library's one documented deviation from :77-78; identical for a batch of one and
for identical binary masks)."""
import numpy as np
from scipy.ndimage import uniform_filter

WIN, K1, K2, DATA_RANGE = 7, 0.01, 0.03, 2.0
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
PAD = (WIN - 1) // 2


def to_range(im):
    """(im * 2 - 1).clamp(-1, 1) in float32 (:48-49)"""
    return np.clip(np.asarray(im, np.float32) * np.float32(2) - np.float32(1), np.float32(-1), np.float32(1))


def margins(h, w, margin):
    return (int(h * margin) + 1, int(w * margin) + 1) if margin > 0 else (0, 0)


def crop(a, mh, mw):
    return a[:, mh:a.shape[1] - mh, mw:a.shape[2] - mw]


def ssim_map(x, y, dtype=np.float64):
    """structural_similarity's S for one channel [h, w] (skimage/metrics/_structural_similarity.py, 0.19.2)"""
    if min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    x, y = x.astype(dtype), y.astype(dtype)
    cov_norm = WIN * WIN / (WIN * WIN - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim_image(x, y, dtype=np.float64):
    """(mssim, S [h, w, 3]) of one image [h, w, 3]: per channel the mean of S over the region shrunk by 3, then the mean over the channels"""
    S = np.stack([ssim_map(x[..., c], y[..., c], dtype) for c in range(x.shape[-1])], -1)
    per_channel = [S[PAD:S.shape[0] - PAD, PAD:S.shape[1] - PAD, c].mean(dtype=np.float64) for c in range(S.shape[-1])]
    return float(np.mean(np.asarray(per_channel, dtype=dtype))), S


def mse_image(x, y, dtype=np.float64):
    return float(np.mean((x.astype(dtype) - y.astype(dtype)) ** 2, dtype=np.float64))


def psnr_image(x, y, dtype=np.float64):
    """peak_signal_noise_ratio(image_true=x, image_test=y) with data_range None: 1 if x has no negative value, else 2"""
    data_range = 1.0 if np.min(x) >= 0 else 2.0
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(data_range ** 2 / np.float64(mse_image(x, y, dtype))))


def img_metrics_ref(pred, target, margin=0, mask=None, dtype=np.float64):
    """pred, target [B, H, W, 3] in (0, 1); mask None or [B, H, W, 1 or 3] -> dict of float64 arrays mse, psnr, ssim [B]"""
    x, y = to_range(pred), to_range(target)
    mh, mw = margins(x.shape[1], x.shape[2], margin)
    m = None
    if mask is not None:
        m = crop(np.broadcast_to(np.asarray(mask, np.float32), x.shape), mh, mw).astype(dtype)
    x, y = crop(x, mh, mw), crop(y, mh, mw)
    out = {"mse": [], "psnr": [], "ssim": []}
    for i in range(x.shape[0]):
        xi, yi = x[i].astype(dtype), y[i].astype(dtype)
        if m is not None:
            xm, ym = xi * m[i], yi * m[i]
            with np.errstate(divide="ignore"):
                corr = 10 * np.log10(x.shape[1] * x.shape[2] / np.float64(m[i, ..., 0].sum(dtype=np.float64)))
            out["mse"].append(mse_image(xm, ym, dtype) - corr)
            out["psnr"].append(psnr_image(xm, ym, dtype) - corr)
            S = ssim_image(xi, yi, dtype)[1]
            out["ssim"].append(float((S * m[i]).sum(dtype=np.float64) / m[i].sum(dtype=np.float64)))
        else:
            out["mse"].append(mse_image(xi, yi, dtype))
            out["psnr"].append(psnr_image(xi, yi, dtype))
            out["ssim"].append(ssim_image(xi, yi, dtype)[0])
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def smooth_images(seed, B, H, W, noise=0.05, overshoot=True):
    """a seeded pair of smooth images plus noise, float32 [B, H, W, 3]: SSIM well inside (0, 1); with `overshoot` some prediction values lie
    outside [0, 1] (the clamp)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = rs.uniform(0, 2 * np.pi, (B, 1, 1, 3))
    fr = rs.uniform(0.15, 0.6, (B, 1, 1, 3))
    base = 0.5 + 0.3 * np.sin(fr * xx[None, ..., None] + ph) * np.cos(0.7 * fr * yy[None, ..., None] - ph)
    target = base + noise * rs.standard_normal(base.shape)
    pred = base + 0.03 * np.cos(0.3 * xx + 0.2 * yy)[None, ..., None] + noise * rs.standard_normal(base.shape)
    if overshoot:
        pick = rs.rand(*base.shape) < 0.04
        pred = np.where(pick, pred + rs.choice([-0.9, 0.9], base.shape), pred)
    return pred.astype(np.float32), np.clip(target, 0, 1).astype(np.float32)
