"""Mirror of the reference's rigid blur kernel network: ``RigidBlurringModel`` (networks/dpnerf/blurmodel.py:9-173) with its
``ViewEmbedding`` (networks/embedding.py:6-32), as run_nerf.py:167-215 builds them.  The module carries the reference's parameter names,
shapes and initialisation, so a reference checkpoint's ``kernelsnet.*`` keys load; its forward and backward are one and two launches of
the library (evd_rigid_blur_forward / _backward) that read the parameters in place."""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import nn

from . import _lib as L

_PARAM_FIELDS = [f for f, _ in L.RigidBlurParams._fields_]


class ViewEmbedding(nn.Module):
    """networks/embedding.py:6-32 ('param' embedding: one learnable row per image)"""

    def __init__(self, num_embed, embed_dim, init_params="zero"):
        super().__init__()
        self.num_embed, self.embed_dim, self.out_channels = num_embed, embed_dim, embed_dim
        if init_params == "zero":
            v = torch.zeros(num_embed, embed_dim)
        elif init_params == "normal":
            v = torch.randn(num_embed, embed_dim)
        elif init_params == "linspace":
            v = torch.linspace(-1, 1, num_embed)[:, None].repeat(1, embed_dim)
        else:
            raise ValueError("Unknown init_params: {}".format(init_params))
        self.img_embed = nn.Parameter(v.float(), True)

    def forward(self, x):
        return self.img_embed[x]


class _RigidBlurFn(torch.autograd.Function):
    """(rays, ids | None, x | None, table | None, twelve network tensors) -> (new_rays, weight, img_embed)"""

    @staticmethod
    def forward(ctx, desc, rays, ids, x, table, *net):
        R = rays.shape[0]
        M, P, Cw = desc.M, desc.M + desc.use_origin, desc.C
        new_rays = torch.empty((R, P, 3, 2), dtype=torch.float32, device=rays.device)
        weight = torch.empty((R, M + 1), dtype=torch.float32, device=rays.device)
        img_embed = torch.empty((R, Cw), dtype=torch.float32, device=rays.device)
        prm = _params(table, net)
        L.check(L.lib().evd_rigid_blur_forward(C.byref(desc), C.byref(prm), L.ptr(rays), L.ptr(ids), L.ptr(x), R, L.ptr(new_rays), L.ptr(weight),
                                               L.ptr(img_embed), L.stream_ptr()), "evd_rigid_blur_forward")
        ctx.desc = desc
        ctx.save_for_backward(rays, ids, x, table, *net)
        ctx.set_materialize_grads(False)
        return new_rays, weight, img_embed

    @staticmethod
    def backward(ctx, d_new_rays, d_weight, d_img_embed):
        desc = ctx.desc
        rays, ids, x, table, *net = ctx.saved_tensors
        R, dev = rays.shape[0], rays.device
        d_new_rays = torch.zeros((R, desc.M + desc.use_origin, 3, 2), device=dev) if d_new_rays is None else d_new_rays.contiguous()
        d_weight = torch.zeros((R, desc.M + 1), device=dev) if d_weight is None else d_weight.contiguous()
        d_img_embed = None if d_img_embed is None else d_img_embed.contiguous()
        sizes = [0 if table is None else table.numel()] + [t.numel() for t in net]
        flat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
        d_rays = torch.empty_like(rays) if ctx.needs_input_grad[1] else None
        d_x = torch.empty_like(x) if x is not None and ctx.needs_input_grad[3] else None
        lib = L.lib()
        need = int(lib.evd_rigid_blur_workspace_bytes(C.byref(desc), R))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
        prm = _params(table, net)
        L.check(lib.evd_rigid_blur_backward(C.byref(desc), C.byref(prm), L.ptr(rays), L.ptr(ids), L.ptr(x), R, L.ptr(d_new_rays), L.ptr(d_weight),
                                            L.ptr(d_img_embed), L.ptr(flat), L.ptr(d_rays), L.ptr(d_x), L.ptr(ws), need, L.stream_ptr()),
                "evd_rigid_blur_backward")
        grads, o = [], 0
        for t, n in zip((table,) + tuple(net), sizes):           # the flat buffer sliced into the leaves' gradients
            grads.append(None if t is None else flat[o:o + n].view(t.shape))
            o += n
        return (None, d_rays, None, d_x, *grads)


def _params(table, net):
    prm = L.RigidBlurParams()
    for f, t in zip(_PARAM_FIELDS, (table,) + tuple(net)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.EvdError(f"RigidBlurKernel: parameter {f} must be contiguous float32")
        setattr(prm, f, None if t is None else t.data_ptr())
    return prm


class RigidBlurKernel(nn.Module):
    """RigidBlurringModel (networks/dpnerf/blurmodel.py:9-49,129-173).  `view_embed`: None builds the 'param' ViewEmbedding of
    run_nerf.py:168-170 (n_imgs x embed_dim), whose rows the kernel gathers itself; any other module (the reference's
    ViewEmbeddingMLP, :171-175) stays PyTorch in front of the kernel and hands it per-ray rows, as does a `feats` input."""

    def __init__(self, n_imgs, embed_dim=32, embed_init="zero", num_motion=9, D_r=1, W_r=32, D_v=1, W_v=32, D_w=1, W_w=32,
                 output_ch_r=3, output_ch_v=3, feat_ch=0, rv_window=0.1, use_origin=True, view_embed=None, use_view_embed=True):
        super().__init__()
        if output_ch_r != 3 or output_ch_v != 3:
            raise L.EvdError("RigidBlurKernel: rotation and translation have three components (output_ch_r = output_ch_v = 3)")
        self.view_embed_module = ViewEmbedding(n_imgs, embed_dim, embed_init) if view_embed is None else view_embed
        self.use_view_embed = use_view_embed
        W = self.view_embed_module.out_channels if use_view_embed else 0
        self.num_motion, self.use_origin, self.rv_window = num_motion, use_origin, rv_window
        self.feat_ch = feat_ch * ((num_motion + 1) if use_origin else num_motion)
        self.output_ch_r = self.output_ch_v = 3 * num_motion
        self.output_ch_w = num_motion

        def branch(D, Wd):
            return nn.ModuleList([nn.Linear(W + self.feat_ch, Wd)] + [nn.Linear(Wd, Wd) for _ in range(D - 1)])

        def head(Wd, out_ch):
            lin = nn.Linear(Wd, out_ch)
            nn.init.xavier_uniform_(lin.weight, gain=0.00001 / math.sqrt((Wd + out_ch) / 6))          # blurmodel.py:38-39: U(-b, b), b = 6e-5 / (Wd + out_ch)
            return lin

        self.r_branch = branch(D_r, W_r)
        self.r_linear = head(W_r, self.output_ch_r)
        self.v_branch = branch(D_v, W_v)
        self.v_linear = head(W_v, self.output_ch_v)
        self.w_branch = branch(D_w, W_w)
        self.w_linear = nn.Linear(W_w, self.output_ch_w + 1)

    @classmethod
    def from_args(cls, args, n_imgs):
        """the constructor call of run_nerf.py:168-170,204-215 ('param' embedding)"""
        kind = getattr(args, "kernel_img_embed_type", "param")
        if kind != "param":
            raise L.EvdError(f"RigidBlurKernel.from_args: kernel_img_embed_type {kind!r}: pass the embedding module as view_embed")
        return cls(n_imgs, embed_dim=args.kernel_img_embed, embed_init=getattr(args, "kernel_img_embed_init", "zero"),
                   num_motion=args.kernel_ptnum - 1, D_r=args.kernel_rbk_se_r_depth, W_r=args.kernel_rbk_se_r_width,
                   D_v=args.kernel_rbk_se_v_depth, W_v=args.kernel_rbk_se_v_width, D_w=args.kernel_rbk_ccw_depth, W_w=args.kernel_rbk_ccw_width,
                   output_ch_r=args.kernel_rbk_se_r_output_ch, output_ch_v=args.kernel_rbk_se_v_output_ch,
                   feat_ch=getattr(args, "kernel_rbk_extra_feat_ch", 0), rv_window=args.kernel_rbk_se_rv_window,
                   use_origin=args.kernel_rbk_use_origin)

    @classmethod
    def from_state_dict(cls, sd, rv_window=0.1, use_origin=True, prefix=""):
        """the module a reference checkpoint's `kernelsnet.*` tensors (prefix 'kernelsnet.') describe, with them loaded"""
        sd = {k[len(prefix):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(prefix)}
        depth = lambda b: len([k for k in sd if k.startswith(f"{b}_branch.") and k.endswith(".weight")])
        n_imgs, embed_dim = sd["view_embed_module.img_embed"].shape
        M = sd["w_linear.weight"].shape[0] - 1
        extra = sd["r_branch.0.weight"].shape[1] - embed_dim
        slots = M + 1 if use_origin else M
        if extra < 0 or extra % slots:
            raise L.EvdError("RigidBlurKernel.from_state_dict: branch input width does not fit the embedding")
        mod = cls(n_imgs, embed_dim=embed_dim, num_motion=M, D_r=depth("r"), W_r=sd["r_branch.0.weight"].shape[0], D_v=depth("v"),
                  W_v=sd["v_branch.0.weight"].shape[0], D_w=depth("w"), W_w=sd["w_branch.0.weight"].shape[0], feat_ch=extra // slots,
                  rv_window=rv_window, use_origin=use_origin)
        mod.load_state_dict(sd)
        return mod

    def _desc(self, Cw, n_img):
        return L.RigidBlurDesc(C=Cw, W_r=self.r_branch[0].out_features, W_v=self.v_branch[0].out_features, W_w=self.w_branch[0].out_features,
                               D_r=len(self.r_branch), D_v=len(self.v_branch), D_w=len(self.w_branch), M=self.num_motion,
                               use_origin=int(bool(self.use_origin)), n_img=n_img, rv_window=float(self.rv_window))

    def forward(self, H, W, K, rays, rays_info, feats=None, return_img_embed=False, **kwargs):
        ids = rays_info["images_idx"].reshape(-1)
        rays = rays.float().contiguous()
        net = (self.r_branch[0].weight, self.r_branch[0].bias, self.v_branch[0].weight, self.v_branch[0].bias, self.w_branch[0].weight,
               self.w_branch[0].bias, self.r_linear.weight, self.r_linear.bias, self.v_linear.weight, self.v_linear.bias, self.w_linear.weight,
               self.w_linear.bias)
        table_form = type(self.view_embed_module) is ViewEmbedding and self.use_view_embed and self.feat_ch == 0
        if table_form:
            table = self.view_embed_module.img_embed
            ids = ids.to(torch.int64).contiguous()
            new_rays, weight, img_embed = _RigidBlurFn.apply(self._desc(table.shape[1], table.shape[0]), rays, ids, None, table, *net)
        else:
            view_feature = self.view_embed_module(ids)
            parts = [view_feature] if self.use_view_embed else []
            if self.feat_ch:
                parts.append(torch.zeros(ids.shape[0], self.feat_ch, device=rays.device) if feats is None else feats.view(ids.shape[0], self.feat_ch))
            x = (parts[0] if len(parts) == 1 else torch.cat(parts, -1)).float().contiguous()
            new_rays, weight, _ = _RigidBlurFn.apply(self._desc(x.shape[1], 0), rays, None, x, None, *net)
            img_embed = view_feature
        return new_rays, weight, None, ({"img_embed": img_embed} if return_img_embed else {})
