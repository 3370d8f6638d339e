"""8-bit pictures of the test-set, video and render-only passes on the GPU: the arithmetic the reference's ``run_nerf.py`` does on the host
between ``render_path`` and its image / video / logger calls.

    depth_images   255 - to8b(disp / max) through a colour map, or to8b(disp / max)       :374,382,385,389  :663,675  :732
    error_maps     ((rgb - gt) ** 2).mean(-1), 255 - to8b(pixmse / pixmse.max()) per frame, through a colour map   :670,679
    video_frames   to8b((rgbs - rgbs.min()) / (rgbs.max() - rgbs.min()))                                             :726,730
    test_set_pass, video_pass   one call per pass (:654-707, :716-733): render_path, the CRF, metrics.compute_img_metric and the pictures

Device tensors in, uint8 device tensors out, two library calls per picture kind (evd_frame_range, evd_frame_map) with the minimum and
maximum handed over in device memory: a pass copies uint8 pictures and a handful of scalars to the host instead of the float32 frames.
Every step is the single float32 operation NumPy performs, in its order, so the bytes are the reference's bit for bit.  Two stated
deviations where the reference's result is undefined: a slice whose maximum is 0 (video RGB: whose maximum equals its minimum) is grey
level 0 throughout, and a NaN pixel is grey level 0 and does not take part in the minimum and maximum.

THE COLOUR TABLE IS THE CALLER'S, like the LPIPS weights: ``colormap`` is a [256, 3] uint8 array or tensor and its rows come back in the
order given (OpenCV's applyColorMap returns BGR; which order the table has is the caller's business).  The reference's table is OpenCV's
COLORMAP_TWILIGHT_SHIFTED (INTEGRATION.md shows the one line that obtains it); nothing is shipped or fetched.  There is no CPU fallback."""
from __future__ import annotations

import torch

from . import _lib as L
from . import metrics as M

SRC_PLAIN, SRC_INVERT, SRC_SQERR = 0, 1, 2          # EVD_FRAME_SRC_* of include/evdnerf.h
SCOPES = {"all": 0, "frame": 1}                      # EVD_FRAME_SCOPE_*


def _table(colormap, what):
    """the caller's table, checked before anything touches the device"""
    if colormap is None:
        return None
    t = torch.as_tensor(colormap)
    if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
        raise L.EvdError(f"{what}: the colour map must be a [256, 3] uint8 table, got {tuple(t.shape)} {t.dtype}")
    return t


def _frames(x, what):
    xx = torch.as_tensor(x).detach().to(torch.float32).contiguous()
    if xx.dim() < 1 or xx.numel() == 0:
        raise L.EvdError(f"{what}: frames of shape {tuple(xx.shape)}")
    return xx


def _on_device(x, what):
    if not x.is_cuda:
        raise L.EvdError(f"{what}: the frames must be on the GPU (there is no CPU fallback)")


def _pictures(x, y, source, scope, n_frames, per_frame, subtract_lo, lut, shape, what):
    """evd_frame_range + evd_frame_map on one stack: uint8 `shape` (+ [3] with a table)"""
    _on_device(x, what)
    lib = L.lib()
    lut = None if lut is None else lut.to(x.device).contiguous()
    need = int(lib.evd_frame_workspace_bytes(n_frames, per_frame, scope))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=x.device)
    rng = torch.empty((2 * (n_frames if scope == SCOPES["frame"] else 1),), dtype=torch.float32, device=x.device)
    out = torch.empty(tuple(shape) + ((3,) if lut is not None else ()), dtype=torch.uint8, device=x.device)
    L.check(lib.evd_frame_range(L.ptr(x), L.ptr(y), source, scope, n_frames, per_frame, L.ptr(rng), L.ptr(ws), need, L.stream_ptr()), f"{what}: evd_frame_range")
    L.check(lib.evd_frame_map(L.ptr(x), L.ptr(y), source, scope, n_frames, per_frame, L.ptr(rng), int(subtract_lo), L.ptr(lut), L.ptr(out), L.stream_ptr()),
            f"{what}: evd_frame_map")
    return out


def depth_images(disps, invert=True, scope="all", colormap=None):
    """disps [N, ...] -> uint8 of the same shape: to8b(d / d.max()) with d = 1 - disps (invert, run_nerf.py:374,663) or disps (:732), the
    maximum over all frames (scope 'all': :389, :675, :732) or per frame ('frame': :382).  With a colour map [N, ..., 3]:
    colormap[255 - to8b(...)], i.e. cv2.applyColorMap(255 - to8b(...), table) (:385, :675)."""
    if scope not in SCOPES:
        raise L.EvdError(f"depth_images: scope '{scope}' ('all' or 'frame')")
    lut = _table(colormap, "depth_images")
    d = _frames(disps, "depth_images")
    n = int(d.shape[0])
    return _pictures(d, None, SRC_INVERT if invert else SRC_PLAIN, SCOPES[scope], n, d.numel() // n, False, lut, d.shape, "depth_images")


def error_maps(rgbs, gts, colormap=None):
    """rgbs, gts [N, H, W, 3] -> uint8 [N, H, W]: to8b(pixmse / pixmse.max()) with pixmse = ((rgb - gt) ** 2).mean(-1) and the maximum of each
    frame (run_nerf.py:670,679); with a colour map [N, H, W, 3]: colormap[255 - to8b(...)].  The error itself is never stored."""
    lut = _table(colormap, "error_maps")
    p = _frames(rgbs, "error_maps")
    t = _frames(gts, "error_maps").to(p.device)
    if p.shape != t.shape or p.dim() < 2 or p.shape[-1] != 3:
        raise L.EvdError(f"error_maps: frames {tuple(p.shape)} and {tuple(t.shape)}: the shapes must match and end in 3")
    n = int(p.shape[0])
    return _pictures(p, t, SRC_SQERR, SCOPES["frame"], n, p.numel() // (3 * n), False, lut, p.shape[:-1], "error_maps")


def video_frames(rgbs):
    """rgbs [N, H, W, 3] -> uint8 of the same shape: to8b((rgbs - rgbs.min()) / (rgbs.max() - rgbs.min())), minimum and maximum over all
    frames (run_nerf.py:726,730)"""
    x = _frames(rgbs, "video_frames")
    return _pictures(x, None, SRC_PLAIN, SCOPES["all"], int(x.shape[0]), x.numel() // int(x.shape[0]), True, None, x.shape, "video_frames")


def apply_colormap(u8, colormap):
    """the bare table lookup colormap[u8]: uint8 [...] -> uint8 [..., 3] (cv2.applyColorMap(u8, table) with the caller's table)"""
    lut = _table(colormap, "apply_colormap")
    if lut is None:
        raise L.EvdError("apply_colormap: a [256, 3] uint8 colour map is required")
    u = torch.as_tensor(u8)
    if u.dtype != torch.uint8:
        raise L.EvdError(f"apply_colormap: a uint8 picture, got {u.dtype}")
    _on_device(u, "apply_colormap")
    u = u.contiguous()
    out = torch.empty(tuple(u.shape) + (3,), dtype=torch.uint8, device=u.device)
    L.check(L.lib().evd_frame_colormap(L.ptr(u), u.numel(), L.ptr(lut.to(u.device).contiguous()), L.ptr(out), L.stream_ptr()), "evd_frame_colormap")
    return out


def _render(model, crf, H, W, K, chunk, poses, render_kwargs):
    """render_path with the poses on the model's device (its frames stay there), then the CRF's encode_rgb"""
    poses = [torch.as_tensor(p, dtype=torch.float32).to(model.device) for p in poses]
    rgbs, disps = model.render_path(H, W, K, chunk, poses, render_kwargs)
    return crf(rgbs, mode="encode_rgb"), disps


def test_set_pass(model, crf, H, W, K, chunk, poses, gts, render_kwargs, colormap=None, metrics=("mse", "psnr", "ssim")):
    """The test-set pass, run_nerf.py:654-707, in one call: render_path, crf(..., mode='encode_rgb'), compute_img_metric for every name in
    `metrics` ('lpips' only where a model is installed with metrics.set_lpips), the predictions' to8b (:673,704), the depth pictures
    (:663,675) and the error maps (:670,679).  Returns a dict: the float32 device frames `rgbs` [N, H, W, 3] and `disps` [N, H, W] (as
    rendered: not inverted), the uint8 device pictures `rgb8`, `gt8` [N, H, W, 3], `depth8`, `err8` ([N, H, W], or [N, H, W, 3] with a
    colour map), and `metrics`, a dict of Python floats."""
    rgbs, disps = _render(model, crf, H, W, K, chunk, poses, render_kwargs)
    gts = torch.as_tensor(gts).to(rgbs.device)
    return {"rgbs": rgbs, "disps": disps,
            "metrics": {m: M.compute_img_metric(rgbs, gts, m) for m in metrics},
            "rgb8": M.to8b(rgbs), "gt8": M.to8b(gts),
            "depth8": depth_images(disps, invert=True, scope="all", colormap=colormap),
            "err8": error_maps(rgbs, gts, colormap=colormap)}


test_set_pass.__test__ = False          # (a library function whose name starts with test_: not a test to collect)


def video_pass(model, crf, H, W, K, chunk, poses, render_kwargs):
    """The video pass, run_nerf.py:716-733: render_path, crf(..., mode='encode_rgb'), the normalised RGB frames (:726,730) and the depth
    frames to8b(disps / disps.max()) (:732).  Returns a dict: float32 device frames `rgbs`, `disps`, uint8 device pictures `rgb8`
    [N, H, W, 3] and `disp8` [N, H, W]."""
    rgbs, disps = _render(model, crf, H, W, K, chunk, poses, render_kwargs)
    return {"rgbs": rgbs, "disps": disps, "rgb8": video_frames(rgbs), "disp8": depth_images(disps, invert=False, scope="all")}
