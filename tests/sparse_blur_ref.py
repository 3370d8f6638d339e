"""float64 restatement of the sparse blur kernel network (BlurModel.forward, networks/pdrf/blurmodel.py:109-224, kernel_type DSK and PBE,
with ViewEmbedding 'param' in front): the reference the tests of csrc/kernel_sparse_blur.hip compare with.  Written from the formulas:

    pt      = tanh(pattern_pos[img]) hwindow + noise random_hwindow                    [R, P, 2]   (input_pos)
    row     = [embed(pt pi / hwindow) | table[img] | feats (PBE) | embed(x / (W / 2 / pi) - pi, y / (H / 2 / pi) - pi)]
    out     = linears1([row, linears(row)] or linears(row))                             [R, P, 3 or 5]  = [delta_trans (sv) | delta_pos | logit]
    trans   = 0.01 (delta_trans or pattern_trans[img] or 0),   xy = delta_pos + pt     (PBE: point 0 of both is 0)
    align   = mean |xy[:, 0]| + 10 mean |trans[:, 0]|                                   (DSK),      weight = softmax_P(logit)
    dirs    = ((x - cx + xy_x) / fx - trans_x, -(y - cy + xy_y) / fy - trans_y, -1),    rays_d = pose[:3, :3] dirs,   rays_o = pose (trans_x, trans_y, 0, 1)

with embed(v) = [v, sin(2^0 v), cos(2^0 v), ..., sin(2^(L-1) v), cos(2^(L-1) v)], every entry on the 2-vector.  Everything is torch in
the dtype of `dtype`, so gradients are torch.autograd's.  tests/test_sparse_blur_ref.py checks this file against the reference's recorded
float32 results (golden G39) within the reference's own float32 error."""
import math

import numpy as np
import torch

G39_CASES = ("dsk", "dsk_full", "dsk_sv", "pbe")
ABSENT_IMAGE = 3          # no ray of a G39 batch belongs to it
ALIGN_C = 0.7             # the fixed factor of align in G39's recorded loss


def embed(v, L):
    out = [v]
    for f in range(L):
        out += [torch.sin(v * 2.0 ** f), torch.cos(v * 2.0 ** f)]
    return torch.cat(out, -1)


def param_keys(cfg, with_poses=False):
    keys = ["pattern_pos"] + (["pattern_trans"] if cfg["optim_trans"] else []) + ["img_embed.img_embed"]
    keys += [f"linears.{2 * i}.{w}" for i in range(cfg["num_hidden"]) for w in ("weight", "bias")]
    keys += [f"linears1.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")]
    return tuple(keys + (["poses"] if with_poses else []))


def forward(p, cfg, H, W, K4, ids, rays_x, rays_y, poses, noise=None, feats=None, x=None):
    """p: the reference's state-dict names -> tensors; K4 = (fx, fy, cx, cy); ids [R]; rays_x, rays_y [R]; poses [R, 3, 4]; noise [R, P, 2] or None;
    feats [R P, feat_cnl] or None; x [R, C] per-ray embedding rows in place of table[ids]
    -> new_rays [R, P, 3, 2], weight [R, P], align (0-d, None for PBE), img_embed [R, C]"""
    P, hw, R = cfg["num_pt"], float(cfg["kernel_hwindow"]), ids.shape[0]
    pick = (lambda a: a.expand(R, -1, -1)) if cfg["isglobal"] else (lambda a: a[ids])
    pt = torch.tanh(pick(p["pattern_pos"])) * hw
    if noise is not None and cfg["random_hwindow"] > 0:
        pt = pt + noise * cfg["random_hwindow"]
    img_embed = p["img_embed.img_embed"][ids] if x is None else x
    cols = [embed(pt * (math.pi / hw), cfg["in_embed"]), img_embed[:, None].expand(R, P, img_embed.shape[-1])]
    if cfg["kernel_type"] == "PBE":
        cols.append(torch.zeros(R, P, cfg["feat_cnl"], dtype=pt.dtype, device=pt.device) if feats is None else feats.reshape(R, P, -1))
    if cfg["spatial_embed"] > 0:
        s = torch.stack([rays_x / (W / 2 / math.pi) - math.pi, rays_y / (H / 2 / math.pi) - math.pi], -1)
        cols.append(embed(s, cfg["spatial_embed"])[:, None].expand(R, P, -1))
    row = torch.cat(cols, -1)
    h = row
    for i in range(cfg["num_hidden"]):
        h = torch.relu(h @ p[f"linears.{2 * i}.weight"].T + p[f"linears.{2 * i}.bias"])
    h = torch.cat([row, h], -1) if cfg["short_cut"] else h
    h = torch.relu(h @ p["linears1.0.weight"].T + p["linears1.0.bias"])
    out = h @ p["linears1.2.weight"].T + p["linears1.2.bias"]
    if cfg["optim_spatialvariant_trans"]:
        trans, dpos, logit = out[..., 0:2], out[..., 2:4], out[..., 4]
    else:
        trans, dpos, logit = None, out[..., 0:2], out[..., 2]
    if cfg["optim_trans"]:
        trans = pick(p["pattern_trans"])
    trans = torch.zeros_like(dpos) if trans is None else trans
    trans = trans * 0.01
    xy = dpos + pt
    if cfg["kernel_type"] == "PBE":
        keep = torch.ones(1, P, 1, dtype=pt.dtype, device=pt.device)
        keep[:, 0] = 0
        xy, trans, align = xy * keep, trans * keep, None
    else:
        align = xy[:, 0].abs().mean() + trans[:, 0].abs().mean() * 10
    weight = torch.softmax(logit, -1)
    fx, fy, cx, cy = K4
    dx = (rays_x[:, None] - cx + xy[..., 0]) / fx - trans[..., 0]
    dy = -(rays_y[:, None] - cy + xy[..., 1]) / fy - trans[..., 1]
    dirs = torch.stack([dx, dy, -torch.ones_like(dx)], -1)
    rays_d = (dirs[..., None, :] * poses[:, None, :3, :3]).sum(-1)
    tr = torch.stack([trans[..., 0], trans[..., 1], torch.zeros_like(dx), torch.ones_like(dx)], -1)
    rays_o = (tr[..., None, :] * poses[:, None]).sum(-1)
    return torch.stack([rays_o, rays_d], -1), weight, align, img_embed


def run(params, cfg, H, W, K4, ids, rays_x, rays_y, poses, noise, proj, feats=None, x=None, d_out=None, dtype=torch.float64):
    """outputs and gradients of  sum(new_rays proj.new_rays) + sum(weight proj.weight) + sum(img_embed proj.img_embed) + ALIGN_C align  on
    float32-valued inputs -- or, with d_out = dict(new_rays, weight[, align][, img_embed]), of the sum of the outputs times those incoming gradients.
    poses None: the module's `poses` buffer (params['poses']) indexed by image.
    -> dict(new_rays, weight, align, img_embed, grads {name: array}[, d_feats][, d_x])"""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    p = {k: T(v).requires_grad_(k != "poses") for k, v in params.items()}
    idt = torch.as_tensor(np.asarray(ids), dtype=torch.long).reshape(-1)
    pose_rows = p["poses"][idt] if poses is None else T(poses)
    leaf_f = None if feats is None else T(feats).requires_grad_(True)
    leaf_x = None if x is None else T(x).requires_grad_(True)
    new_rays, weight, align, img_embed = forward(p, cfg, H, W, K4, idt, T(rays_x).reshape(-1), T(rays_y).reshape(-1), pose_rows,
                                                 None if noise is None else T(noise), leaf_f, leaf_x)
    if d_out is not None:
        loss = (new_rays * T(d_out["new_rays"])).sum() + (weight * T(d_out["weight"])).sum()
        if align is not None and d_out.get("align") is not None:
            loss = loss + align * float(np.asarray(d_out["align"]).reshape(-1)[0])
        if d_out.get("img_embed") is not None:
            loss = loss + (img_embed * T(d_out["img_embed"])).sum()
    else:
        loss = (new_rays * T(proj["new_rays"])).sum() + (weight * T(proj["weight"])).sum() + (img_embed * T(proj["img_embed"])).sum()
        if align is not None:
            loss = loss + ALIGN_C * align
    names = [k for k in p if k != "poses" and (x is None or k != "img_embed.img_embed")]
    leaves = [p[k] for k in names] + [l for l in (leaf_f, leaf_x) if l is not None]
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves)]
    out = dict(new_rays=new_rays.detach().numpy(), weight=weight.detach().numpy(), align=None if align is None else align.detach().numpy(),
               img_embed=img_embed.detach().numpy(), grads={k: gi.numpy() for k, gi in zip(names, g)})
    rest = list(g[len(names):])
    if leaf_f is not None:
        out["d_feats"] = rest.pop(0).numpy()
    if leaf_x is not None:
        out["d_x"] = rest.pop(0).numpy()
    return out


def g39_case(g, tag):
    """one case of golden G39 -> dict(cfg, H, W, K4, params, ids, rays_x, rays_y, poses | None, noise | None, feats | None, proj {..}, out {..}, grads {..}
    (the reference's float32 results), err_out {..}, err_g {..} (its float32 error against itself in float64))"""
    pre = tag + "."
    pick = lambda sub: {k[len(pre + sub):]: g[k] for k in g if k.startswith(pre + sub)}
    cfg = {k: (str(v) if k == "kernel_type" else float(v) if k in ("random_hwindow",) else int(v)) for k, v in pick("cfg.").items()}
    opt = lambda k: g[pre + k] if pre + k in g else None
    return dict(cfg=cfg, H=400, W=400, K4=tuple(float(v) for v in g[pre + "K4"]), params=pick("sd."), ids=g[pre + "ids"].reshape(-1),
                rays_x=g[pre + "rays_x"], rays_y=g[pre + "rays_y"], poses=opt("poses"), noise=opt("noise"), feats=opt("feats"), proj=pick("proj."),
                out=pick("out."), grads=pick("g."), err_out={k: float(v) for k, v in pick("ref_f32_err.out.").items()},
                err_g={k: float(v) for k, v in pick("ref_f32_err.g.").items()})


_G39_REF = {}


def g39_reference(g, tag):
    """run() on a G39 case, computed once per process and shared by the tests (treat the arrays as read-only)"""
    if tag not in _G39_REF:
        c = g39_case(g, tag)
        _G39_REF[tag] = run(c["params"], c["cfg"], c["H"], c["W"], c["K4"], c["ids"], c["rays_x"], c["rays_y"], c["poses"], c["noise"], c["proj"],
                            feats=c["feats"])
    return _G39_REF[tag]


def subset(c, idx):
    """the rays `idx` of a case: (ids, rays_x, rays_y, poses, noise, feats, proj)"""
    P = c["cfg"]["num_pt"]
    rows = (np.asarray(idx)[:, None] * P + np.arange(P)).reshape(-1)
    sel = lambda a: None if a is None else a[idx]
    return dict(ids=c["ids"][idx], rays_x=c["rays_x"][idx], rays_y=c["rays_y"][idx], poses=sel(c["poses"]), noise=sel(c["noise"]),
                feats=None if c["feats"] is None else c["feats"][rows], proj={k: v[idx] for k, v in c["proj"].items()})


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
