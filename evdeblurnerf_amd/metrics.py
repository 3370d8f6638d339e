"""Image metrics of the test-set pass on the GPU: mirror of the reference ``utils/metrics.py`` (compute_img_metric :18-100 for 'mse',
'psnr' and 'ssim', img2mse :7, mse2psnr :8) and of ``to8b`` (utils/misc.py:6).  The three metrics of a batch of frames come from one library
call (evd_img_metrics) without a host copy; scikit-image is not needed.  The arithmetic after the reference's float32 mapping is float64.

One deliberate deviation: with a mask, every image is multiplied by its own mask.  The reference multiplies the whole batch by every earlier
image's mask inside its loop (:77-78); the two agree for a batch of one and for identical binary masks.

LPIPS (:92-95, networks/lpips/lpips.py) runs on the device in float32 (evd_lpips, evd_lpips_spatial), eval mode: the AlexNet backbone (the
reference's ``LPIPS()`` call) or VGG-16 (``net='vgg'``, the variant most papers report), version 0.1 or 0.0, with the linear heads or as
the baseline without them (``lpips=False``), as the spatial average or as the spatial map (``spatial=True``).  Its WEIGHTS ARE THE
CALLER'S: a backbone's pretrained weights are not part of the reference checkout (torchvision downloads them), so ``LPIPS`` is built from
state dicts or files the user already has, nothing is ever downloaded, and ``compute_img_metric(..., 'lpips')`` works once a model is
installed with ``set_lpips``.  net='squeeze', dropout in training mode, pnet_tune and any backward are not built."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L
from .losses import img2mse  # noqa: F401  (utils/metrics.py:7)
from .weights import LPIPS_VGG16

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


class LPIPS:
    """The reference's ``LPIPS(net, version, lpips, spatial)`` in eval mode (dropout is the identity) on the device.
    backbone: torchvision's state dict of the backbone -- AlexNet ``features.{0,3,6,8,10}.{weight,bias}`` for net='alex', VGG-16
    ``features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}`` for net='vgg' / 'vgg16'; other keys such as ``classifier.*`` are ignored;
    lin: the linear heads (``lin{0..4}.model.1.weight``, the keys of the reference's weights/v0.1/{alex,vgg}.pth), required with lpips=True and
    ignored with lpips=False (the baseline: the plain channel sum);
    version: '0.1', or '0.0' without the scaling layer;
    spatial: the call returns the per-pixel map [B, 1, H, W] instead of the per-image value.  The library packs the weights once."""
    CONV = ((0, 3, 64, 11), (3, 64, 192, 5), (6, 192, 384, 3), (8, 384, 256, 3), (10, 256, 256, 3))       # features index, Cin, Cout, kernel
    CONV_VGG = tuple((idx, ci, co, 3) for idx, ci, co in LPIPS_VGG16)
    CHNS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}                          # lpips.py:159-164
    SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)                                             # ScalingLayer, lpips.py:245-252

    def __init__(self, backbone, lin=None, net="alex", version="0.1", lpips=True, spatial=False):
        if net == "squeeze":
            raise NotImplementedError("LPIPS: net='squeeze' is not built: its fire modules have 16-, 32- and 48-channel layers, channel "
                                      "concatenation and ceil-mode pools, none of which fit the convolution kernel's 64-column tile")
        if net not in ("alex", "vgg", "vgg16"):
            raise L.EvdError(f"LPIPS: net '{net}'; 'alex', 'vgg' or 'vgg16'")
        if version not in ("0.1", "0.0"):
            raise L.EvdError(f"LPIPS: version '{version}'; '0.1' or '0.0' (the original release without the scaling layer)")
        if lpips and lin is None:
            raise L.EvdError("LPIPS: lpips=True needs the linear heads (lin); lpips=False is the baseline without them")
        net = "alex" if net == "alex" else "vgg"
        name = "the AlexNet" if net == "alex" else "the VGG-16"
        self.net, self.version, self.lpips, self.spatial = net, version, bool(lpips), bool(spatial)

        def take(sd, key, shape, what):
            if key not in sd:
                raise L.EvdError(f"LPIPS: {what} state dict has no '{key}'")
            v = torch.as_tensor(sd[key]).detach().to(device="cpu", dtype=torch.float32)
            if v.numel() != math.prod(shape) or (v.dim() == len(shape) and tuple(v.shape) != shape):
                raise L.EvdError(f"LPIPS: '{key}' has shape {tuple(v.shape)}, expected {shape}")
            return v.reshape(shape).contiguous()

        keep = []
        desc = L.LpipsNetDesc()
        desc.net, desc.heads = (L.LPIPS_NET_ALEX if net == "alex" else L.LPIPS_NET_VGG16), int(self.lpips)
        for l, (idx, ci, co, k) in enumerate(self.CONV if net == "alex" else self.CONV_VGG):
            w = take(backbone, f"features.{idx}.weight", (co, ci, k, k), name)
            b = take(backbone, f"features.{idx}.bias", (co,), name)
            keep += [w, b]
            desc.conv_w[l] = ctypes.cast(w.data_ptr(), L._fp)
            desc.conv_b[l] = ctypes.cast(b.data_ptr(), L._fp)
        for l, co in enumerate(self.CHNS[net] if self.lpips else ()):
            h = take(lin, f"lin{l}.model.1.weight", (1, co, 1, 1), "the linear-head")
            keep.append(h)
            desc.lin[l] = ctypes.cast(h.data_ptr(), L._fp)
        for c in range(3):                                           # version 0.0: no scaling layer; (x - 0) / 1 is exact
            desc.shift[c], desc.scale[c] = (self.SHIFT[c], self.SCALE[c]) if version == "0.1" else (0.0, 1.0)
        self._lib = L.lib()
        self._h = ctypes.c_void_p()
        L.check(self._lib.evd_lpips_create_net(ctypes.byref(desc), ctypes.byref(self._h)), "evd_lpips_create_net")

    @classmethod
    def from_files(cls, backbone_path, lin_path=None, **kwargs):
        """The files are read with torch.load(..., map_location='cpu', weights_only=True); nothing is downloaded."""
        lin = None if lin_path is None else torch.load(lin_path, map_location="cpu", weights_only=True)
        return cls(torch.load(backbone_path, map_location="cpu", weights_only=True), lin, **kwargs)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.evd_lpips_destroy(h)

    def _inputs(self, im1, im2, format):
        p = _bhwc(im1, format)
        t = _bhwc(im2, format).to(p.device)
        if not p.is_cuda:
            raise L.EvdError("LPIPS: the images must be on the GPU (there is no CPU fallback)")
        if p.shape != t.shape:
            raise L.EvdError(f"LPIPS: shapes {tuple(p.shape)} and {tuple(t.shape)} differ")
        B, H, W = (int(v) for v in p.shape[:3])
        need = int(self._lib.evd_lpips_model_workspace_bytes(self._h, B, H, W, int(self.spatial)))
        return p, t, B, H, W, need, torch.empty((max(need, 1),), dtype=torch.uint8, device=p.device)

    def _run(self, im1, im2, format):
        if self.spatial:
            raise L.EvdError("LPIPS: a spatial model returns a map per image, not a value: build one with spatial=False for the mean")
        p, t, B, H, W, need, ws = self._inputs(im1, im2, format)
        out = torch.empty((6 * B + 1,), dtype=torch.float64, device=p.device)
        L.check(self._lib.evd_lpips(self._h, L.ptr(p), L.ptr(t), B, H, W, L.ptr(out), L.ptr(ws), need, L.stream_ptr()), "evd_lpips")
        return out, B

    def _run_spatial(self, im1, im2, format, layers):
        p, t, B, H, W, need, ws = self._inputs(im1, im2, format)
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=p.device)
        per = torch.empty((B, 5, H, W), dtype=torch.float32, device=p.device) if layers else None
        L.check(self._lib.evd_lpips_spatial(self._h, L.ptr(p), L.ptr(t), B, H, W, L.ptr(out), L.ptr(per), L.ptr(ws), need, L.stream_ptr()),
                "evd_lpips_spatial")
        return out, per

    def __call__(self, im1, im2, format=None, retPerLayer=False):
        """im1, im2 in (0, 1), laid out as compute_img_metric takes them -> the [B] float64 device tensor of per-image values, and with
        retPerLayer the [B, 5] per-layer terms (each layer's own term: the reference's list carries the total in slot 0 because its sum adds
        in place).  A spatial model returns the float32 map [B, 1, H, W] (the reference's shape), and with retPerLayer the five upsampled
        per-layer maps [B, 5, H, W].  No host copy, no synchronisation."""
        if self.spatial:
            out, per = self._run_spatial(im1, im2, format, retPerLayer)
            return (out, per) if retPerLayer else out
        out, B = self._run(im1, im2, format)
        return (out[:B], out[B + 1:].view(B, 5)) if retPerLayer else out[:B]

    def mean(self, im1, im2, format=None):
        """the batch mean, summed image by image (0-dim float64 device tensor); not for a spatial model"""
        out, B = self._run(im1, im2, format)
        return out[B]


_LPIPS = [None]


def set_lpips(model):
    """Install the LPIPS model compute_img_metric(..., 'lpips') uses (the reference's module-level `photometric` cache, utils/metrics.py:11-16,
    filled by hand because the weights are the caller's); None removes it."""
    if model is not None and not isinstance(model, LPIPS):
        raise L.EvdError(f"set_lpips: an evdeblurnerf_amd.metrics.LPIPS or None, got {type(model).__name__}")
    if model is not None and getattr(model, "spatial", False):
        raise L.EvdError("set_lpips: a spatial LPIPS model returns maps; compute_img_metric needs one built with spatial=False")
    _LPIPS[0] = model


def compute_img_metric(im1t, im2t, metric="mse", margin=0, mask=None, format=None):
    """utils/metrics.py:18-100: the mean of `metric` over the batch as a Python float (one read-back).  im1t, im2t: batched images in (0, 1),
    [H, W, 3], [3, H, W], [B, H, W, 3] or [B, 3, H, W] (`format` None, 'HWC', 'CHW', 'BHWC'; anything else means [B, 3, H, W]).
    'lpips' needs a model installed with set_lpips and IGNORES margin and mask, as the reference's branch does: it feeds the un-cropped,
    un-masked im1t[i:i+1] to the network (:92-95)."""
    if metric not in PHOTOMETRIC:
        raise RuntimeError(f"img_utils:: metric {metric} not recognized")
    if metric == "lpips":
        if _LPIPS[0] is None:
            raise NotImplementedError("compute_img_metric: 'lpips' needs the LPIPS backbone's pretrained weights, which are not part of the "
                                      "reference checkout and cannot be fetched: build metrics.LPIPS from the backbone and linear-head weights "
                                      "you have and install it with metrics.set_lpips; 'mse', 'psnr' and 'ssim' run on the device")
        return float(_LPIPS[0].mean(im1t, im2t, format=format))
    return float(img_metrics(im1t, im2t, margin=margin, mask=mask, format=format)[metric + "_mean"])


def to8b(x):
    """utils/misc.py:6, (255 * np.clip(x, 0, 1)).astype(np.uint8), on a device tensor: uint8 of the same shape (NaN -> 0)"""
    xx = x.detach().to(torch.float32).contiguous()
    if not xx.is_cuda:
        raise L.EvdError("to8b: the tensor must be on the GPU (there is no CPU fallback)")
    out = torch.empty(xx.shape, dtype=torch.uint8, device=xx.device)
    L.check(L.lib().evd_to8b(L.ptr(xx), xx.numel(), L.ptr(out), L.stream_ptr()), "evd_to8b")
    return out
