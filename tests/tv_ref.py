"""float64 reference of the TV regulariser of one PDRF level (TV_loss_app, voxnerf.py:126-130 over TVLoss :306-324), of its gradient in
closed form, and of the quantity that scales the rounding-error bound of a float32 gradient.  Test infrastructure only.

Layout: the library's channel-last grids, planes [H, W, C] and lines [L, 1, C] (a line is a plane of width 1: its width term is empty and
its count is clamped to 1, as torch_restatement.torch_tv does), all float64.

  reg(x)       = 2 (sum_h (x[h+1] - x[h])^2 / count_h + sum_w (x[:, w+1] - x[:, w])^2 / count_w),
                 count_h = C (H - 1) W,  count_w = max(C H (W - 1), 1)
  value        = sum_i reg(plane_i) 1e-2 + reg(line_i) 1e-3
  d reg / d x  = kh ((c - up) - (down - c)) + kw ((c - left) - (right - c)),  kh = 4 / count_h,  kw = 4 / count_w, a neighbour outside the
                 tensor contributing nothing
  A            = |kh| (|c - up| + |down - c|) + |kw| (|c - left| + |right - c|): the sum of the absolute values of the terms a kernel adds,
                 so a float32 evaluation with n roundings per term is within n 2^-24 A of the exact gradient, element by element.
An axis of size 1 along H is not defined (the reference divides by zero)."""
import torch

PLANE_W, LINE_W = 1e-2, 1e-3


def _counts(x):
    H, W, C = x.shape
    if H < 2:
        raise ValueError("tv_ref: the first axis must have at least 2 entries (the reference divides by C (H - 1) W)")
    return float(C * (H - 1) * W), float(max(C * H * (W - 1), 1))


def reg(x):
    """TVLoss.forward of one channel-last tensor [H, W, C] (weight 1, batch 1)"""
    ch, cw = _counts(x)
    dh, dw = x[1:] - x[:-1], x[:, 1:] - x[:, :-1]
    return 2 * ((dh ** 2).sum() / ch + (dw ** 2).sum() / cw)


def value(planes, lines):
    """(a): the level's TV value from three planes [H, W, C] and three lines [L, 1, C]"""
    return sum(reg(p) * PLANE_W + reg(l) * LINE_W for p, l in zip(planes, lines))


def grad(x, scale=1.0):
    """(b) and (c) for one tensor: (scale d reg / d x, A), both [H, W, C]; `scale` = upstream scalar x the tensor's weight"""
    ch, cw = _counts(x)
    kh, kw = 4.0 * scale / ch, 4.0 * scale / cw
    dh, dw = x[1:] - x[:-1], x[:, 1:] - x[:, :-1]
    g, a = torch.zeros_like(x), torch.zeros_like(x)
    g[1:] += kh * dh
    g[:-1] -= kh * dh
    g[:, 1:] += kw * dw
    g[:, :-1] -= kw * dw
    a[1:] += abs(kh) * dh.abs()
    a[:-1] += abs(kh) * dh.abs()
    a[:, 1:] += abs(kw) * dw.abs()
    a[:, :-1] += abs(kw) * dw.abs()
    return g, a


def level_grad(planes, lines, upstream=1.0):
    """(b), (c) for the six tensors in the library's order (planes 0..2, lines 0..2): ([gradients], [A])"""
    out = [grad(p, upstream * PLANE_W) for p in planes] + [grad(l, upstream * LINE_W) for l in lines]
    return [g for g, _ in out], [a for _, a in out]


def from_state_dict(sd, prefix=""):
    """reference layouts (app_plane.i [1, C, H, W], app_line.i [1, C, L, 1]) -> (planes [H, W, C], lines [L, 1, C]) in float64"""
    t = lambda k: torch.as_tensor(sd[prefix + k]).double()[0].permute(1, 2, 0).contiguous()
    return [t(f"app_plane.{i}") for i in range(3)], [t(f"app_line.{i}") for i in range(3)]


def edge_mask(x):
    """first and last row, first and last column of [H, W, C]"""
    m = torch.zeros(x.shape, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m
