"""Float64 yardstick of the LPIPS metric for both backbones and every built option, written from its formulas, for any weights (what is
shared with the AlexNet-only restatement is imported from tests/lpips_ref.py):

    x        = (clamp(2 im - 1, -1, 1) - shift) / scale                    the clamp in float32 (utils/metrics.py:48-49), the rest in `dtype`;
                                                                           version 0.0 is shift 0, scale 1
    backbone   a list of convolutions (features index, kernel, stride, pad, pool in front, tap), each followed by a ReLU:
               'alex'  features[0:12] of AlexNet: 11 x 11 / 4, 5 x 5, 3 x 3 x 3; max pool 3 x 3 / stride 2 (floor) in front of the second
                       and third; every convolution is a tap
               'vgg'   features[0:30] of VGG-16: thirteen 3 x 3 / pad 1 convolutions, 64, 64, 128, 128, 256 x 3, 512 x 3, 512 x 3 channels;
                       max pool 2 x 2 / stride 2 (floor) in front of convolutions 2, 4, 7, 10; taps after 1, 3, 6, 9, 12
    n        = sqrt(sum_c f_c^2)                                            per pixel and frame, at every tap
    d_l      = sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2    per pixel; the baseline (lins None) has lin_c = 1
    term_l   = mean over pixels of d_l;   value = sum_l term_l
    map_l    = d_l resampled to H x W bilinearly: output pixel o reads the source coordinate s = max((o + 0.5) in / out - 0.5, 0) in each
               axis, i0 = floor(s), i1 = min(i0 + 1, in - 1), weights 1 - (s - i0) and s - i0;   map = sum_l map_l in layer order

Convolutions and pools run over explicit patches (unfold, then a matrix product / a maximum).  Torch on the CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

from lpips_ref import EPS, _conv, map_input

# features index, kernel, stride, pad, (pool window, pool stride) in front or None, tap
NETS = {
    "alex": ((0, 11, 4, 2, None, True), (3, 5, 1, 2, (3, 2), True), (6, 3, 1, 1, (3, 2), True), (8, 3, 1, 1, None, True), (10, 3, 1, 1, None, True)),
    "vgg": tuple((idx, 3, 1, 1, (2, 2) if idx in (5, 10, 17, 24) else None, idx in (2, 7, 14, 21, 28))
                 for idx in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)),
}


def pool(x, win, stride):
    """max over win x win windows, floor mode: every window lies inside the map"""
    B, C, H, W = x.shape
    ho, wo = (H - win) // stride + 1, (W - win) // stride + 1
    return F.unfold(x, win, stride=stride).reshape(B, C, win * win, ho * wo).max(dim=2).values.reshape(B, C, ho, wo)


def features(x, backbone, net, dtype=torch.float64):
    """the five tapped feature maps of the mapped and scaled frames x [B, 3, H, W]"""
    outs = []
    h = x
    for idx, k, stride, pad, pl, tap in NETS[net]:
        if pl is not None:
            h = pool(h, *pl)
        w = torch.as_tensor(np.asarray(backbone[f"features.{idx}.weight"])).to(dtype)
        b = torch.as_tensor(np.asarray(backbone[f"features.{idx}.bias"])).to(dtype)
        h = torch.relu(_conv(h, w, b, k, stride, pad))
        if tap:
            outs.append(h)
    return outs


def _axis(n_in, n_out, dtype):
    s = torch.clamp((torch.arange(n_out, dtype=dtype) + 0.5) * (n_in / n_out) - 0.5, min=0.0)
    i0 = torch.clamp(s.floor().long(), max=n_in - 1)
    return i0, torch.clamp(i0 + 1, max=n_in - 1), s - i0.to(dtype)


def upsample(d, H, W):
    """d [B, h, w] -> [B, H, W], bilinear, half-pixel centres (align_corners=False)"""
    y0, y1, ly = _axis(d.shape[1], H, d.dtype)
    x0, x1, lx = _axis(d.shape[2], W, d.dtype)
    r0 = (1 - lx) * d[:, y0][:, :, x0] + lx * d[:, y0][:, :, x1]
    r1 = (1 - lx) * d[:, y1][:, :, x0] + lx * d[:, y1][:, :, x1]
    return (1 - ly)[None, :, None] * r0 + ly[None, :, None] * r1


def distances(pred, target, backbone, lins, shift, scale, net, dtype=torch.float64):
    """the five per-pixel distance maps d_l [B, h_l, w_l] and (H, W)"""
    sh = torch.as_tensor(np.asarray(shift, dtype=np.float32)).to(dtype).reshape(1, 3, 1, 1)
    sc = torch.as_tensor(np.asarray(scale, dtype=np.float32)).to(dtype).reshape(1, 3, 1, 1)
    x0, x1 = map_input(pred).to(dtype), map_input(target).to(dtype)
    f0 = features((x0 - sh) / sc, backbone, net, dtype)
    f1 = features((x1 - sh) / sc, backbone, net, dtype)
    ds = []
    for l, (a, b) in enumerate(zip(f0, f1)):
        na = torch.sqrt((a ** 2).sum(dim=1, keepdim=True))
        nb = torch.sqrt((b ** 2).sum(dim=1, keepdim=True))
        d = (a / (na + EPS) - b / (nb + EPS)) ** 2
        if lins is not None:
            d = d * torch.as_tensor(np.asarray(lins[l])).to(dtype).reshape(1, -1, 1, 1)
        ds.append(d.sum(dim=1))
    return ds, tuple(x0.shape[2:])


def _sum_in_order(parts):
    total = parts[0].clone()
    for p in parts[1:]:
        total = total + p
    return total


def lpips(pred, target, backbone, lins, shift, scale, net="vgg", dtype=torch.float64):
    """pred, target: [B, H, W, 3] (or [H, W, 3]) float32 frames in (0, 1); backbone: torchvision's state dict of `net`; lins: five vectors, or
    None for the baseline; shift, scale: [3].  Returns (value [B], terms [B, 5]) as float64 numpy arrays."""
    ds, _ = distances(pred, target, backbone, lins, shift, scale, net, dtype)
    terms = [d.mean(dim=(1, 2)) for d in ds]
    return _sum_in_order(terms).double().numpy(), torch.stack(terms, dim=1).double().numpy()


def lpips_spatial(pred, target, backbone, lins, shift, scale, net="vgg", dtype=torch.float64):
    """as lpips(); returns (map [B, H, W], layer_maps [B, 5, H, W]) as float64 numpy arrays"""
    ds, (H, W) = distances(pred, target, backbone, lins, shift, scale, net, dtype)
    maps = [upsample(d, H, W) for d in ds]
    return _sum_in_order(maps).double().numpy(), torch.stack(maps, dim=1).double().numpy()
