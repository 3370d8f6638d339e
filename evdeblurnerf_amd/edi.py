"""Event double integral prior on the GPU: mirror of the reference ``utils/edi.py``
(brightness_increment_image :44-70 with bilinear splat :7-41, deblur_double_integral :91-95), and the prior table built from them,
``LLFFEventsDataset.compute_edi_prior`` (data/loader_events.py:99-131), in one call."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def brightness_increment_image(x, y, p, w, h, c_pos, c_neg, interpolate=True, color_events=False):
    if color_events:
        raise NotImplementedError("Bayer demosaicing of colour events (cv2.cvtColor) is CPU data preparation")
    if not interpolate:
        x, y = torch.floor(x), torch.floor(y)
    x, y = x.contiguous().float(), y.contiguous().float()
    p = p.contiguous().to(torch.int8)
    img = torch.empty((h, w), dtype=torch.float32, device=x.device)
    L.check(L.lib().evd_edi_bii_image(L.ptr(x), L.ptr(y), L.ptr(p), x.shape[0], int(w), int(h), float(c_pos), float(c_neg),
                                      L.ptr(img), L.stream_ptr()), "evd_edi_bii_image")
    return img


def deblur_double_integral(blurry, bii):
    """blurry [H,W(,3)], bii [steps-1, H,W(,3)] -> sharp, utils/edi.py:91-95."""
    b = blurry.contiguous().float()
    e = bii.contiguous().float()
    out = torch.empty_like(b)
    L.check(L.lib().evd_edi_deblur(L.ptr(b), L.ptr(e), e.shape[0] + 1, b.numel(), L.ptr(out), L.stream_ptr()), "evd_edi_deblur")
    return out


def compute_edi_prior(events, id_to_coords, tms_start, tms_end, images, steps, cpos, cneg, return_windows=False, chunk=None, check=True):
    """LLFFEventsDataset.compute_edi_prior (data/loader_events.py:99-131) on device tensors: events [N, 4] float64 (id, t, p, successor),
    id_to_coords [Ncoords, 2] float64, tms_start / tms_end [n] (host, the units of the events' timestamps), images [n, H, W, 3] ->
    the sharpened images [n, H, W, 3] float32 (and, with return_windows, left / right int64 [n, steps]: the searchsorted indices of :111-112).
    The boundaries are np.linspace on the host in float64, as the reference makes them.  chunk: images per pass (None: as many as the
    library's cap takes; the result does not depend on it).  check=True reads the device flag back and raises for a coordinate id
    outside id_to_coords."""
    ts = np.asarray(tms_start, dtype=np.float64).reshape(-1)
    te = np.asarray(tms_end, dtype=np.float64).reshape(-1)
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[-1] != 3 or img.shape[0] != ts.shape[0] or te.shape[0] != ts.shape[0]:
        raise L.EvdError("compute_edi_prior: images [n, H, W, 3] and one start / end timestamp per image")
    dev = events.device
    ev = events.contiguous().to(torch.float64)
    i2c = id_to_coords.contiguous().to(torch.float64)
    if ev.dim() != 2 or ev.shape[1] != 4 or i2c.dim() != 2 or i2c.shape[1] != 2:
        raise L.EvdError("compute_edi_prior: events [N, 4] and id_to_coords [Ncoords, 2]")
    img = img.to(device=dev, dtype=torch.float32).contiguous()
    n, h, w = (int(v) for v in img.shape[:3])
    out = torch.empty_like(img)
    win = torch.empty((2, n, int(steps)), dtype=torch.int64, device=dev) if return_windows else None
    if n == 0:
        return (out, win[0], win[1]) if return_windows else out
    bounds = torch.as_tensor(np.stack([np.linspace(a, b, int(steps)) for a, b in zip(ts, te)]), device=dev).contiguous()
    lib = L.lib()
    need = int(lib.evd_edi_prior_workspace_bytes(n if chunk is None else max(1, min(int(chunk), n)), int(steps), h, w))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(lib.evd_edi_prior(L.ptr(ev), ev.shape[0], L.ptr(i2c), i2c.shape[0], L.ptr(bounds), L.ptr(img), n, int(steps), h, w, float(cpos), float(cneg),
                              L.ptr(out), L.ptr(win), L.ptr(bad), L.ptr(ws), need, L.stream_ptr()), "evd_edi_prior")
    if check and int(bad.item()):
        raise L.EvdError("compute_edi_prior: an event's coordinate id lies outside id_to_coords")
    return (out, win[0], win[1]) if return_windows else out
