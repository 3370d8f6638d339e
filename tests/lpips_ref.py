"""Float64 yardstick of the LPIPS metric (AlexNet backbone, version 0.1, linear heads, spatial average, eval mode), written from its formulas,
for any weights:

    x        = (clamp(2 im - 1, -1, 1) - shift) / scale                    the clamp in float32 (utils/metrics.py:48-49), the rest in `dtype`
    f_1      = relu(conv(x;   11 x 11, stride 4, pad 2,   3 ->  64))
    f_2      = relu(conv(pool(f_1); 5 x 5, pad 2,        64 -> 192))       pool = max over 3 x 3, stride 2, floor
    f_3      = relu(conv(pool(f_2); 3 x 3, pad 1,       192 -> 384))
    f_4      = relu(conv(f_3; 3 x 3, pad 1,             384 -> 256))
    f_5      = relu(conv(f_4; 3 x 3, pad 1,             256 -> 256))
    n        = sqrt(sum_c f_c^2)                                            per pixel and frame
    term_l   = mean over pixels of sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2
    value    = sum_l term_l

Convolutions and pools run over explicit patches (unfold, then a matrix product / a maximum).  Torch on the CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ((0, 11, 4, 2, False), (3, 5, 1, 2, True), (6, 3, 1, 1, True), (8, 3, 1, 1, False), (10, 3, 1, 1, False))   # features index, k, stride, pad, pool first
EPS = 1e-10


def _conv(x, w, b, k, stride, pad):
    B, _, H, W = x.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    patches = F.unfold(x, k, padding=pad, stride=stride)                   # [B, Cin k k, ho wo], rows ordered (c, ky, kx) as the weight's
    y = torch.matmul(w.reshape(w.shape[0], -1), patches) + b[None, :, None]
    return y.reshape(B, -1, ho, wo)


def _pool(x):
    B, C, H, W = x.shape
    ho, wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    return F.unfold(x, 3, stride=2).reshape(B, C, 9, ho * wo).max(dim=2).values.reshape(B, C, ho, wo)


def map_input(im):
    """[..., H, W, 3] float32 in (0, 1) -> clamp(2 im - 1, -1, 1) in float32, [B, 3, H, W]"""
    im = torch.as_tensor(np.asarray(im, dtype=np.float32))
    if im.dim() == 3:
        im = im[None]
    return (im * 2 - 1).clamp(-1, 1).permute(0, 3, 1, 2)


def features(x, backbone, dtype=torch.float64):
    """the five feature maps of the mapped and scaled frames x [B, 3, H, W]"""
    outs = []
    h = x
    for idx, k, stride, pad, pool in LAYERS:
        if pool:
            h = _pool(h)
        w = torch.as_tensor(np.asarray(backbone[f"features.{idx}.weight"])).to(dtype)
        b = torch.as_tensor(np.asarray(backbone[f"features.{idx}.bias"])).to(dtype)
        h = torch.relu(_conv(h, w, b, k, stride, pad))
        outs.append(h)
    return outs


def lpips(pred, target, backbone, lins, shift, scale, dtype=torch.float64):
    """pred, target: [B, H, W, 3] (or [H, W, 3]) float32 frames in (0, 1); backbone: features.{0,3,6,8,10}.{weight,bias}; lins: five vectors;
    shift, scale: [3].  Returns (value [B], terms [B, 5]) as float64 numpy arrays."""
    sh = torch.as_tensor(np.asarray(shift, dtype=np.float32)).to(dtype).reshape(1, 3, 1, 1)
    sc = torch.as_tensor(np.asarray(scale, dtype=np.float32)).to(dtype).reshape(1, 3, 1, 1)
    f0 = features((map_input(pred).to(dtype) - sh) / sc, backbone, dtype)
    f1 = features((map_input(target).to(dtype) - sh) / sc, backbone, dtype)
    terms = []
    for a, b, lin in zip(f0, f1, lins):
        na = torch.sqrt((a ** 2).sum(dim=1, keepdim=True))
        nb = torch.sqrt((b ** 2).sum(dim=1, keepdim=True))
        d = (a / (na + EPS) - b / (nb + EPS)) ** 2
        w = torch.as_tensor(np.asarray(lin)).to(dtype).reshape(1, -1, 1, 1)
        terms.append((d * w).sum(dim=1).mean(dim=(1, 2)))
    terms = torch.stack(terms, dim=1)
    value = terms[:, 0].clone()
    for l in range(1, terms.shape[1]):
        value = value + terms[:, l]
    return value.double().numpy(), terms.double().numpy()
