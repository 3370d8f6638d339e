"""Image metrics of the test-set pass on the GPU: mirror of the reference ``utils/metrics.py`` (compute_img_metric :18-100 for 'mse',
'psnr' and 'ssim', img2mse :7, mse2psnr :8) and of ``to8b`` (utils/misc.py:6).  The three metrics of a batch of frames come from one library
call (evd_img_metrics) without a host copy; scikit-image is not needed.  The arithmetic after the reference's float32 mapping is float64.

One deliberate deviation: with a mask, every image is multiplied by its own mask.  The reference multiplies the whole batch by every earlier
image's mask inside its loop (:77-78); the two agree for a batch of one and for identical binary masks.

LPIPS is not built: its AlexNet backbone weights are not part of the reference checkout (torchvision downloads them)."""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .losses import img2mse  # noqa: F401  (utils/metrics.py:7)

TILE_H, TILE_W = 16, 32          # EVD_IMG_METRICS_TILE_H / _W of include/evdnerf.h: the kernel's tile of output pixels
PHOTOMETRIC = ("mse", "ssim", "psnr", "lpips")


def mse2psnr(x):
    """utils/metrics.py:8"""
    return -10. * torch.log(x) / math.log(10.)


def _bhwc(im, format):
    """the reference's layout handling (:51-65): 3-D input gets a batch axis; channels-last if the last axis is 3 (format None) or the
    format says so, else [B, C, H, W]"""
    if (im.dim() == 3 and format is None) or format in ("HWC", "CHW"):
        im = im.unsqueeze(0)
    if im.dim() != 4:
        raise L.EvdError(f"img_metrics: images of shape {tuple(im.shape)} (format {format})")
    if not ((im.shape[-1] == 3 and format is None) or format in ("BHWC", "HWC")):
        im = im.permute(0, 2, 3, 1)
    if im.shape[-1] != 3:
        raise L.EvdError(f"img_metrics: three channels expected, got {im.shape[-1]} (format {format})")
    return im.detach().to(torch.float32).contiguous()


def _mask_bhwc(mask, dev):
    """:35-40: [B, H, W], [B, 1, H, W] or [B, 3, H, W] -> [B, H, W, Cm] (a one-channel mask is not expanded: the kernel reads it three times)"""
    mask = torch.as_tensor(mask)
    if mask.dim() == 3:
        mask = mask.unsqueeze(1)
    if mask.dim() != 4 or mask.shape[1] not in (1, 3):
        raise L.EvdError(f"img_metrics: mask of shape {tuple(mask.shape)}; [B, H, W], [B, 1, H, W] or [B, 3, H, W]")
    return mask.detach().permute(0, 2, 3, 1).to(device=dev, dtype=torch.float32).contiguous()


def img_metrics(pred, target, margin=0, mask=None, format=None):
    """MSE, PSNR and SSIM of a batch as compute_img_metric defines them, in one library call: a dict of float64 device tensors, `mse`, `psnr`,
    `ssim` [B] and `mse_mean`, `psnr_mean`, `ssim_mean` (0-dim).  pred is the reference's first argument (its minimum picks PSNR's
    data_range).  No host copy, no synchronisation."""
    p = _bhwc(pred, format)
    t = _bhwc(target, format).to(p.device)
    if not p.is_cuda:
        raise L.EvdError("img_metrics: the images must be on the GPU (there is no CPU fallback)")
    if p.shape != t.shape:
        raise L.EvdError(f"img_metrics: shapes {tuple(p.shape)} and {tuple(t.shape)} differ")
    B, H, W = (int(v) for v in p.shape[:3])
    m = None if mask is None else _mask_bhwc(mask, p.device)
    if m is not None and tuple(m.shape[:3]) != (B, H, W):
        raise L.EvdError(f"img_metrics: mask {tuple(m.shape)} for images {tuple(p.shape)}")
    mh, mw = (int(H * margin) + 1, int(W * margin) + 1) if margin > 0 else (0, 0)
    lib = L.lib()
    need = int(lib.evd_img_metrics_workspace_bytes(B, H, W))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=p.device)
    out = torch.empty((3 * B + 3,), dtype=torch.float64, device=p.device)
    L.check(lib.evd_img_metrics(L.ptr(p), L.ptr(t), L.ptr(m), 0 if m is None else int(m.shape[-1]), B, H, W, mh, mw, L.ptr(out), L.ptr(ws), need,
                                L.stream_ptr()), "evd_img_metrics")
    return {"mse": out[:B], "psnr": out[B:2 * B], "ssim": out[2 * B:3 * B], "mse_mean": out[3 * B], "psnr_mean": out[3 * B + 1],
            "ssim_mean": out[3 * B + 2]}


def compute_img_metric(im1t, im2t, metric="mse", margin=0, mask=None, format=None):
    """utils/metrics.py:18-100: the mean of `metric` over the batch as a Python float (one read-back).  im1t, im2t: batched images in (0, 1),
    [H, W, 3], [3, H, W], [B, H, W, 3] or [B, 3, H, W] (`format` None, 'HWC', 'CHW', 'BHWC'; anything else means [B, 3, H, W])."""
    if metric not in PHOTOMETRIC:
        raise RuntimeError(f"img_utils:: metric {metric} not recognized")
    if metric == "lpips":
        raise NotImplementedError("compute_img_metric: 'lpips' is not built: the LPIPS backbone's pretrained weights are not part of the "
                                  "reference checkout and cannot be fetched; 'mse', 'psnr' and 'ssim' run on the device")
    return float(img_metrics(im1t, im2t, margin=margin, mask=mask, format=format)[metric + "_mean"])


def to8b(x):
    """utils/misc.py:6, (255 * np.clip(x, 0, 1)).astype(np.uint8), on a device tensor: uint8 of the same shape (NaN -> 0)"""
    xx = x.detach().to(torch.float32).contiguous()
    if not xx.is_cuda:
        raise L.EvdError("to8b: the tensor must be on the GPU (there is no CPU fallback)")
    out = torch.empty(xx.shape, dtype=torch.uint8, device=xx.device)
    L.check(L.lib().evd_to8b(L.ptr(xx), xx.numel(), L.ptr(out), L.stream_ptr()), "evd_to8b")
    return out
