"""float64 restatement of the rigid blur kernel network (RigidBlurringModel.forward, networks/dpnerf/blurmodel.py:129-173, with
ViewEmbedding 'param' in front and SE3Field / RigidBody of utils/rigid_warping.py behind): the reference the tests of
csrc/kernel_rigid_blur.hip compare with.  Written for all motions at once, not as the reference's loop: with rho = rot, tau = trans,
theta = |rho| + 1e-10 and K = skew(rho) the reference's exp_se3 of the screw axis (rho, tau) / theta is

    R = I + a K + b K K,   p = (I + b K + c K K) tau,   a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2, c = (theta - sin(theta)) / theta^3

and a warped ray is (R o + p, R d).  Below theta = 0.1 the three coefficients come from their power series (float64 loses seven digits
of 1 - cos(theta) at theta = 1e-4 too; the series' first neglected term is 1e-21 of the value there), above it from the closed forms.
Everything is torch, so gradients are torch.autograd's.  tests/test_rigid_blur_ref.py checks this file against the reference's
recorded float32 results (golden G37) within the reference's own float32 error."""
import math

import torch

PARAM_KEYS = ("view_embed_module.img_embed", "r_branch.0.weight", "r_branch.0.bias", "v_branch.0.weight", "v_branch.0.bias",
              "w_branch.0.weight", "w_branch.0.bias", "r_linear.weight", "r_linear.bias", "v_linear.weight", "v_linear.bias",
              "w_linear.weight", "w_linear.bias")
SERIES_BELOW = 0.1


def _series(t, first, terms=7):
    """sum_k (-1)^k t^k / (first + 2 k)!  with t = theta^2:  first = 3 -> c, first = 2 -> b, first = 1 -> a"""
    out = torch.zeros_like(t)
    for k in reversed(range(terms)):
        out = out * t + (-1.0) ** k / math.factorial(first + 2 * k)
    return out


def se3_coefficients(theta):
    t = theta * theta
    small = theta < SERIES_BELOW
    safe = torch.where(small, torch.ones_like(theta), theta)            # keeps the unused branch's gradient finite
    a = torch.where(small, _series(t, 1), torch.sin(safe) / safe)
    b = torch.where(small, _series(t, 2), (1.0 - torch.cos(safe)) / safe ** 2)
    c = torch.where(small, _series(t, 3), (safe - torch.sin(safe)) / safe ** 3)
    return a, b, c


def skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def warp(rays, r, v, M, use_origin):
    """rays [R,3,2]; r, v [R, 3 M] (component-major: column k M + i is component k of motion i) -> new_rays [R, P, 3, 2]"""
    R = rays.shape[0]
    rho, tau = r.reshape(R, 3, M).transpose(1, 2), v.reshape(R, 3, M).transpose(1, 2)          # [R, M, 3]
    theta = torch.linalg.norm(rho, dim=-1) + 1.0e-10
    a, b, c = (x[..., None, None] for x in se3_coefficients(theta))
    K = skew(rho)
    KK = K @ K
    eye = torch.eye(3, dtype=rays.dtype, device=rays.device)
    rot = eye + a * K + b * KK
    p = ((eye + b * K + c * KK) @ tau[..., None])[..., 0]
    o, d = rays[:, None, :, 0], rays[:, None, :, 1]
    wo = (rot @ o[..., None].expand(R, M, 3, 1))[..., 0] + p
    wd = (rot @ d[..., None].expand(R, M, 3, 1))[..., 0]
    out = torch.stack([wo, wd], -1)
    return torch.cat([rays[:, None], out], 1) if use_origin else out


def forward(params, rays, x, M, use_origin, rv_window):
    """params: the reference's state-dict names -> tensors; x [R, C] the rays' feature rows (table[ids] for ViewEmbedding 'param').
    -> new_rays [R, P, 3, 2], weight [R, M + 1]"""
    lin = lambda name, h: h @ params[name + ".weight"].T + params[name + ".bias"]
    hid = {b: torch.relu(lin(f"{b}_branch.0", x)) for b in "rvw"}
    r, v = lin("r_linear", hid["r"]) * rv_window, lin("v_linear", hid["v"]) * rv_window
    s = torch.sigmoid(lin("w_linear", hid["w"]))
    weight = s / (s.sum(-1, keepdim=True) + 1.0e-10)
    return warp(rays, r, v, M, use_origin), weight


def run(params, rays, ids, M, use_origin, rv_window, proj_new_rays, proj_weight, proj_img_embed=None, x=None, dtype=torch.float64):
    """outputs and gradients, in `dtype`, of  sum(new_rays * proj_new_rays) + sum(weight * proj_weight) (+ sum(img_embed * proj_img_embed))
    on float32-valued inputs.  ids: image ids [R] (table form) or None with per-ray rows x.
    -> dict(new_rays, weight, img_embed, grads {name: array}, d_rays, d_x (per-ray form))"""
    T = lambda a: torch.tensor(a, dtype=dtype)
    p = {k: T(v).requires_grad_(True) for k, v in params.items()}
    rays_t = T(rays).requires_grad_(True)
    if ids is not None:
        feat = p["view_embed_module.img_embed"][torch.as_tensor(ids, dtype=torch.long).reshape(-1)]
        leaf_x = None
    else:
        feat = leaf_x = T(x).requires_grad_(True)
    new_rays, weight = forward(p, rays_t, feat, M, use_origin, rv_window)
    loss = (new_rays * T(proj_new_rays)).sum() + (weight * T(proj_weight)).sum()
    if proj_img_embed is not None:
        loss = loss + (feat * T(proj_img_embed)).sum()
    leaves = [v for k, v in p.items() if ids is not None or k != PARAM_KEYS[0]] + [rays_t] + ([leaf_x] if leaf_x is not None else [])
    names = [k for k in p if ids is not None or k != PARAM_KEYS[0]]
    g = torch.autograd.grad(loss, leaves)
    out = dict(new_rays=new_rays.detach().numpy(), weight=weight.detach().numpy(), img_embed=feat.detach().numpy(),
               grads={k: gi.numpy() for k, gi in zip(names, g)}, d_rays=g[len(names)].numpy())
    if leaf_x is not None:
        out["d_x"] = g[-1].numpy()
    return out


G37_CASES = ("regular", "small", "odd")
ABSENT_IMAGE = 3          # no ray of a G37 batch belongs to it


def g37_case(g, tag):
    """one case of golden G37 -> dict(params, rays, ids [R], M, use_origin, rv_window, proj {..}, out {..}, grads {..} (the reference's
    float32 results; grads include 'rays'), err_out {..}, err_g {..} (its float32 error against itself in float64))"""
    pre = tag + "."
    pick = lambda sub: {k[len(pre + sub):]: g[k] for k in g if k.startswith(pre + sub)}
    M, use_origin = (int(v) for v in g[pre + "args"])
    return dict(params=pick("sd."), rays=g[pre + "rays"], ids=g[pre + "ids"].reshape(-1), M=M, use_origin=bool(use_origin),
                rv_window=float(g[pre + "rv_window"]), proj=pick("proj."), out=pick("out."), grads=pick("g."),
                err_out={k: float(v) for k, v in pick("ref_f32_err.out.").items()}, err_g={k: float(v) for k, v in pick("ref_f32_err.g.").items()})


_G37_REF = {}


def g37_reference(g, tag):
    """run() on a G37 case, computed once per process and shared by the tests (treat the arrays as read-only)"""
    if tag not in _G37_REF:
        c = g37_case(g, tag)
        _G37_REF[tag] = run(c["params"], c["rays"], c["ids"], c["M"], c["use_origin"], c["rv_window"], c["proj"]["new_rays"], c["proj"]["weight"],
                            c["proj"]["img_embed"])
    return _G37_REF[tag]


def rel_l2(a, b):
    import numpy as np
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
