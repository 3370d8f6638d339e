"""Mirrors of the reference's blur kernel networks, with its ``ViewEmbedding`` and ``ViewEmbeddingMLP`` (networks/embedding.py:6-62), as
run_nerf.py:167-215 builds them: ``RigidBlurKernel`` for ``RigidBlurringModel`` (networks/dpnerf/blurmodel.py:9-173, kernel_type RBK) and ``SparseBlurKernel`` for
``BlurModel`` (networks/pdrf/blurmodel.py:9-224, kernel_type DSK and PBE).  A module carries the reference's parameter names, shapes and
initialisation, so a reference checkpoint's ``kernelsnet.*`` keys load; its forward and backward are launches of the library
(evd_rigid_blur_* / evd_sparse_blur_* / evd_view_embed_mlp_*) that read the parameters in place."""
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


class _ViewEmbedMlpFn(torch.autograd.Function):
    """(img_embed, the D layers' weights and biases) -> feature table [n_img, W]"""

    @staticmethod
    def forward(ctx, desc, table, *net):
        out = torch.empty((desc.n_img, desc.W), dtype=torch.float32, device=table.device)
        prm = _view_embed_params(table, net)
        L.check(L.lib().evd_view_embed_mlp_forward(C.byref(desc), C.byref(prm), L.ptr(out), L.stream_ptr()), "evd_view_embed_mlp_forward")
        ctx.desc = desc
        ctx.save_for_backward(table, *net)
        return out

    @staticmethod
    def backward(ctx, d_out):
        desc = ctx.desc
        table, *net = ctx.saved_tensors
        leaves = (table,) + tuple(net)
        flat = torch.empty((sum(t.numel() for t in leaves),), dtype=torch.float32, device=table.device)
        lib = L.lib()
        need = int(lib.evd_view_embed_mlp_workspace_bytes(C.byref(desc)))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=table.device)
        prm = _view_embed_params(table, net)
        L.check(lib.evd_view_embed_mlp_backward(C.byref(desc), C.byref(prm), L.ptr(d_out.float().contiguous()), L.ptr(flat), L.ptr(ws), need,
                                                L.stream_ptr()), "evd_view_embed_mlp_backward")
        grads, o = [], 0
        for t in leaves:                                         # the flat buffer sliced into the leaves' gradients
            grads.append(flat[o:o + t.numel()].view(t.shape))
            o += t.numel()
        return (None, *grads)


def _view_embed_params(table, net):
    prm = L.ViewEmbedMlpParams()
    for name, t in (("img_embed", table),) + tuple((f"view_embed_linears[{i // 2}]", t) for i, t in enumerate(net)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.EvdError(f"ViewEmbeddingMLP: parameter {name} must be contiguous float32")
    prm.table = table.data_ptr()
    for i in range(min(len(net) // 2, 8)):                       # (a deeper network is refused by the library: D)
        prm.w[i], prm.b[i] = net[2 * i].data_ptr(), net[2 * i + 1].data_ptr()
    return prm


class ViewEmbeddingMLP(ViewEmbedding):
    """networks/embedding.py:35-62 ('param_mlp': the per-image row through a ReLU MLP, the row concatenated in front of a skip layer's
    output).  The MLP's input depends on the image only, so `feature_table()` evaluates it once per image on the device
    (evd_view_embed_mlp_*); the blur kernel modules gather from that table by image id."""

    def __init__(self, D, W, skips, num_embed, embed_dim, init_params="zero"):
        super().__init__(num_embed, embed_dim, init_params)
        self.D, self.W, self.skips, self.out_channels = D, W, skips, W
        self.view_embed_linears = nn.ModuleList([nn.Linear(embed_dim, W)] +
                                                [nn.Linear(W + embed_dim if i in skips else W, W) for i in range(D - 1)])

    def _desc(self):
        mask = sum(1 << int(i) for i in set(self.skips) if 0 <= int(i) < 32)
        return L.ViewEmbedMlpDesc(n_img=self.img_embed.shape[0], embed_dim=self.img_embed.shape[1], W=self.W, D=len(self.view_embed_linears), skip_mask=mask)

    def feature_table(self):
        """[num_embed, W]: row i = the module's value for image i"""
        net = tuple(t for m in self.view_embed_linears for t in (m.weight, m.bias))
        return _ViewEmbedMlpFn.apply(self._desc(), self.img_embed, *net)

    def forward(self, x):
        return self.feature_table()[x]

    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        """the module that the tensors `<prefix>img_embed`, `<prefix>view_embed_linears.*` describe (not loaded): D, W and E from the shapes,
        the skips from the layers that are E + W wide"""
        num_embed, E = sd[prefix + "img_embed"].shape
        D = len([k for k in sd if k.startswith(prefix + "view_embed_linears.") and k.endswith(".weight")])
        W = sd[prefix + "view_embed_linears.0.weight"].shape[0]
        skips = [i - 1 for i in range(1, D) if sd[f"{prefix}view_embed_linears.{i}.weight"].shape[1] == E + W]
        return cls(D, W, skips, num_embed, E)


def _embedding_from_args(args, n_imgs, who):
    """run_nerf.py:168-175: the 'param' ViewEmbedding (None: the kernel module builds it) or the 'param_mlp' ViewEmbeddingMLP"""
    kind = getattr(args, "kernel_img_embed_type", "param")
    if kind == "param":
        return None
    if kind == "param_mlp":
        return ViewEmbeddingMLP(D=args.kernel_img_mlp_depth, W=args.kernel_img_mlp_embed, skips=[args.kernel_img_mlp_skips], num_embed=n_imgs,
                                embed_dim=args.kernel_img_embed, init_params=getattr(args, "kernel_img_embed_init", "zero"))
    raise L.EvdError(f"{who}.from_args: kernel_img_embed_type {kind!r}: pass the embedding module as view_embed")


def _feature_table(module):
    """the table a blur kernel entry gathers from by image id: the 'param' rows themselves, or the 'param_mlp' module's per-image values"""
    return module.feature_table() if type(module) is ViewEmbeddingMLP else module.img_embed


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
    run_nerf.py:168-170 (n_imgs x embed_dim), whose rows the kernel gathers itself; a ViewEmbeddingMLP of this module ('param_mlp',
    :171-175) is evaluated once per image and the kernel gathers from that table; a module of any other type stays PyTorch in front of
    the kernel and hands it per-ray rows, as does a `feats` input."""

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
        """the constructor call of run_nerf.py:168-175,204-215 ('param' and 'param_mlp' embeddings)"""
        return cls(n_imgs, embed_dim=args.kernel_img_embed, embed_init=getattr(args, "kernel_img_embed_init", "zero"),
                   num_motion=args.kernel_ptnum - 1, D_r=args.kernel_rbk_se_r_depth, W_r=args.kernel_rbk_se_r_width,
                   D_v=args.kernel_rbk_se_v_depth, W_v=args.kernel_rbk_se_v_width, D_w=args.kernel_rbk_ccw_depth, W_w=args.kernel_rbk_ccw_width,
                   output_ch_r=args.kernel_rbk_se_r_output_ch, output_ch_v=args.kernel_rbk_se_v_output_ch,
                   feat_ch=getattr(args, "kernel_rbk_extra_feat_ch", 0), rv_window=args.kernel_rbk_se_rv_window,
                   use_origin=args.kernel_rbk_use_origin, view_embed=_embedding_from_args(args, n_imgs, "RigidBlurKernel"))

    @classmethod
    def from_state_dict(cls, sd, rv_window=0.1, use_origin=True, prefix=""):
        """the module a reference checkpoint's `kernelsnet.*` tensors (prefix 'kernelsnet.') describe, with them loaded"""
        sd = {k[len(prefix):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(prefix)}
        depth = lambda b: len([k for k in sd if k.startswith(f"{b}_branch.") and k.endswith(".weight")])
        n_imgs, embed_dim = sd["view_embed_module.img_embed"].shape
        mlp = ViewEmbeddingMLP.from_state_dict(sd, "view_embed_module.") if "view_embed_module.view_embed_linears.0.weight" in sd else None
        M = sd["w_linear.weight"].shape[0] - 1
        extra = sd["r_branch.0.weight"].shape[1] - (mlp.out_channels if mlp else embed_dim)
        slots = M + 1 if use_origin else M
        if extra < 0 or extra % slots:
            raise L.EvdError("RigidBlurKernel.from_state_dict: branch input width does not fit the embedding")
        mod = cls(n_imgs, embed_dim=embed_dim, num_motion=M, D_r=depth("r"), W_r=sd["r_branch.0.weight"].shape[0], D_v=depth("v"),
                  W_v=sd["v_branch.0.weight"].shape[0], D_w=depth("w"), W_w=sd["w_branch.0.weight"].shape[0], feat_ch=extra // slots,
                  rv_window=rv_window, use_origin=use_origin, view_embed=mlp)
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
        table_form = type(self.view_embed_module) in (ViewEmbedding, ViewEmbeddingMLP) and self.use_view_embed and self.feat_ch == 0
        if table_form:
            table = _feature_table(self.view_embed_module)
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


class _SparseBlurFn(torch.autograd.Function):
    """(ids, x | None, rays_x, rays_y, poses, noise | None, feats | None, pattern_pos, pattern_trans | None, table | None, the linears' and
    linears1's weights and biases) -> (new_rays, weight, align [1] | None, img_embed)"""

    @staticmethod
    def forward(ctx, desc, ids, x, rays_x, rays_y, poses, noise, feats, pattern_pos, pattern_trans, table, *net):
        R, P, dev = ids.shape[0], desc.num_pt, rays_x.device
        new_rays = torch.empty((R, P, 3, 2), dtype=torch.float32, device=dev)
        weight = torch.empty((R, P), dtype=torch.float32, device=dev)
        img_embed = torch.empty((R, desc.embed_cnl), dtype=torch.float32, device=dev)
        align = torch.zeros((1,), dtype=torch.float32, device=dev) if desc.kernel_type == 0 else None
        ws = torch.empty((max(2 * R, 1),), dtype=torch.float32, device=dev) if desc.kernel_type == 0 else None
        prm = _sparse_params(pattern_pos, pattern_trans, table, net)
        L.check(L.lib().evd_sparse_blur_forward(C.byref(desc), C.byref(prm), L.ptr(ids), L.ptr(x), L.ptr(rays_x), L.ptr(rays_y), L.ptr(poses), L.ptr(noise),
                                                L.ptr(feats), R, L.ptr(new_rays), L.ptr(weight), L.ptr(align), L.ptr(img_embed), L.ptr(ws),
                                                0 if ws is None else 4 * ws.numel(), L.stream_ptr()), "evd_sparse_blur_forward")
        ctx.desc = desc
        ctx.save_for_backward(ids, x, rays_x, rays_y, poses, noise, feats, pattern_pos, pattern_trans, table, *net)
        ctx.set_materialize_grads(False)
        return new_rays, weight, align, img_embed

    @staticmethod
    def backward(ctx, d_new_rays, d_weight, d_align, d_img_embed):
        desc = ctx.desc
        ids, x, rays_x, rays_y, poses, noise, feats, pattern_pos, pattern_trans, table, *net = ctx.saved_tensors
        R, P, dev = ids.shape[0], desc.num_pt, rays_x.device
        d_new_rays = torch.zeros((R, P, 3, 2), device=dev) if d_new_rays is None else d_new_rays.contiguous()
        d_weight = torch.zeros((R, P), device=dev) if d_weight is None else d_weight.contiguous()
        d_align = None if d_align is None else d_align.contiguous()
        d_img_embed = None if d_img_embed is None else d_img_embed.contiguous()
        leaves = (pattern_pos, pattern_trans, table) + tuple(net)
        sizes = [0 if t is None else t.numel() for t in leaves]
        flat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
        d_x = torch.empty_like(x) if x is not None and ctx.needs_input_grad[2] else None
        d_feats = torch.empty_like(feats) if feats is not None and ctx.needs_input_grad[7] else None
        lib = L.lib()
        need = int(lib.evd_sparse_blur_workspace_bytes(C.byref(desc), R))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
        prm = _sparse_params(pattern_pos, pattern_trans, table, net)
        L.check(lib.evd_sparse_blur_backward(C.byref(desc), C.byref(prm), L.ptr(ids), L.ptr(x), L.ptr(rays_x), L.ptr(rays_y), L.ptr(poses), L.ptr(noise),
                                             L.ptr(feats), R, L.ptr(d_new_rays), L.ptr(d_weight), L.ptr(d_align), L.ptr(d_img_embed), L.ptr(flat),
                                             L.ptr(d_x), L.ptr(d_feats), L.ptr(ws), need, L.stream_ptr()), "evd_sparse_blur_backward")
        grads, o = [], 0
        for t, n in zip(leaves, sizes):                          # the flat buffer sliced into the leaves' gradients
            grads.append(None if t is None else flat[o:o + n].view(t.shape))
            o += n
        return (None, None, d_x, None, None, None, None, d_feats, *grads)


def _sparse_params(pattern_pos, pattern_trans, table, net):
    prm = L.SparseBlurParams()
    for name, t in (("pattern_pos", pattern_pos), ("pattern_trans", pattern_trans), ("table", table)) + tuple((f"net[{i}]", t) for i, t in enumerate(net)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.EvdError(f"SparseBlurKernel: parameter {name} must be contiguous float32")
    prm.pattern_pos, prm.pattern_trans, prm.table = (None if t is None else t.data_ptr() for t in (pattern_pos, pattern_trans, table))
    hidden = (len(net) - 4) // 2
    for i in range(min(hidden, 4)):                              # (a deeper network is refused by the library: num_hidden)
        prm.linears_w[i], prm.linears_b[i] = net[2 * i].data_ptr(), net[2 * i + 1].data_ptr()
    for i in range(2):
        prm.linears1_w[i], prm.linears1_b[i] = net[2 * hidden + 2 * i].data_ptr(), net[2 * hidden + 2 * i + 1].data_ptr()
    return prm


def init_linear_weights(m):
    """utils/misc.py:95-102: Xavier-normal (gain 0.1 for a weight of 2 or 3 output rows), biases 0"""
    if isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight, 0.1 if m.weight.shape[0] in (2, 3) else 1.0)
        nn.init.constant_(m.bias, 0)


class SparseBlurKernel(nn.Module):
    """BlurModel (networks/pdrf/blurmodel.py:9-224), kernel_type 'DSK' or 'PBE', under the reference's argument names and defaults.
    `view_embed`: None builds the 'param' ViewEmbedding of run_nerf.py:168-170 (num_img x view_embed_cnl, `embed_init`), whose rows the kernel
    gathers itself; a ViewEmbeddingMLP of this module ('param_mlp', :171-175; view_embed_cnl = its W) is evaluated once per image and the kernel
    gathers from that table; a module of any other type stays PyTorch in front of the kernel and hands it per-ray rows.  `noise` of forward is the [R, P, 2]
    standard-normal draw the reference takes with randn_like (in eval mode too); None draws it on the device when random_hwindow > 0."""
    TILE_ROWS = 16            # a tile of the kernels holds TILE_ROWS // num_pt whole rays
    GRID_CAP = 128            # ... and at most this many workgroups share a batch's tiles

    def __init__(self, num_img, num_pt, kernel_hwindow, kernel_type, view_embed=None, img_wh=None, random_hwindow=0.25, in_embed=3, random_mode="input",
                 view_embed_cnl=32, spatial_embed=0, depth_embed=0, num_hidden=3, num_wide=64, feat_cnl=15, short_cut=False, pattern_init_radius=0.1,
                 isglobal=False, optim_trans=False, optim_spatialvariant_trans=False, use_pattern_pos=True, poses=None, embed_init="zero"):
        super().__init__()
        if kernel_type not in ("DSK", "PBE"):
            raise L.EvdError(f"SparseBlurKernel: kernel_type {kernel_type!r} is neither 'DSK' nor 'PBE'")
        if random_mode not in ("input", "output"):
            raise L.EvdError(f"SparseBlurKernel: random_mode {random_mode!r} unrecognized, should be input / output")
        if depth_embed > 0:
            raise L.EvdError("SparseBlurKernel: depth_embed > 0 is not built (the reference calls it deprecated; nothing produces rays_info['ray_depth'])")
        if not use_pattern_pos:
            raise L.EvdError("SparseBlurKernel: use_pattern_pos=False is not built (run_nerf.py never passes it)")
        self.num_pt, self.num_img, self.short_cut, self.kernel_hwindow = num_pt, num_img, short_cut, kernel_hwindow
        self.random_hwindow, self.random_mode, self.kernel_type, self.isglobal, self.feat_cnl = random_hwindow, random_mode, kernel_type, isglobal, feat_cnl
        self.in_embed, self.spatial_embed, self.num_hidden, self.num_wide = in_embed, spatial_embed, num_hidden, num_wide
        self.optim_trans, self.optim_sv_trans = optim_trans, optim_spatialvariant_trans
        pattern_num = 1 if isglobal else num_img
        if poses is not None:
            self.register_buffer("poses", torch.as_tensor(poses).float())
        else:
            self.poses = None
        self.pattern_pos = nn.Parameter(torch.randn(pattern_num, num_pt, 2).float() * pattern_init_radius, True)
        if optim_trans:
            self.pattern_trans = nn.Parameter(torch.zeros(pattern_num, num_pt, 2).float(), True)
        self.img_embed = ViewEmbedding(num_img, view_embed_cnl, embed_init) if view_embed is None else view_embed
        self.img_embed_cnl = view_embed_cnl
        width = lambda L_: 2 * (1 + 2 * L_) if L_ > 0 else 0
        in_cnl = width(in_embed) + view_embed_cnl + width(spatial_embed) + (feat_cnl if kernel_type == "PBE" else 0)
        out_cnl = 5 if optim_spatialvariant_trans else 3
        hiddens = [nn.Linear(num_wide, num_wide) if i % 2 == 0 else nn.ReLU() for i in range((num_hidden - 1) * 2)]
        self.linears = nn.Sequential(nn.Linear(in_cnl, num_wide), nn.ReLU(), *hiddens)
        self.linears1 = nn.Sequential(nn.Linear((num_wide + in_cnl) if short_cut else num_wide, num_wide), nn.ReLU(), nn.Linear(num_wide, out_cnl))
        self.linears.apply(init_linear_weights)
        self.linears1.apply(init_linear_weights)

    @classmethod
    def from_args(cls, args, n_imgs, poses=None):
        """the constructor call of run_nerf.py:168-175,184-203 ('param' and 'param_mlp' embeddings)"""
        view_embed = _embedding_from_args(args, n_imgs, "SparseBlurKernel")
        return cls(n_imgs, args.kernel_ptnum, args.kernel_hwindow, args.kernel_type, random_hwindow=args.kernel_random_hwindow,
                   in_embed=args.kernel_rand_embed, random_mode=args.kernel_random_mode, spatial_embed=args.kernel_spatial_embed,
                   depth_embed=args.kernel_depth_embed, num_hidden=args.kernel_num_hidden, num_wide=args.kernel_num_wide, feat_cnl=args.kernel_feat_cnl,
                   short_cut=args.kernel_shortcut, pattern_init_radius=args.kernel_pattern_init_radius, isglobal=args.kernel_isglobal,
                   optim_trans=args.kernel_global_trans, optim_spatialvariant_trans=args.kernel_spatialvariant_trans,
                   view_embed_cnl=args.kernel_img_embed if view_embed is None else view_embed.out_channels,
                   embed_init=getattr(args, "kernel_img_embed_init", "zero"), poses=poses, view_embed=view_embed)

    @classmethod
    def from_state_dict(cls, sd, kernel_type, kernel_hwindow, random_hwindow=0.25, in_embed=3, spatial_embed=0, isglobal=None, random_mode="input", prefix=""):
        """the module a reference checkpoint's `kernelsnet.*` tensors (prefix 'kernelsnet.') describe, with them loaded.  The tensors fix every
        size but the two embedding depths (and, when there is one image, isglobal): those are arguments."""
        sd = {k[len(prefix):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith(prefix)}
        num_img, embed = sd["img_embed.img_embed"].shape
        mlp = ViewEmbeddingMLP.from_state_dict(sd, "img_embed.") if "img_embed.view_embed_linears.0.weight" in sd else None
        embed = mlp.out_channels if mlp else embed
        n_pat, num_pt, _ = sd["pattern_pos"].shape
        isglobal = (n_pat == 1 and num_img != 1) if isglobal is None else isglobal
        num_wide, in_cnl = sd["linears.0.weight"].shape
        num_hidden = len([k for k in sd if k.startswith("linears.") and k.endswith(".weight")])
        width = lambda L_: 2 * (1 + 2 * L_) if L_ > 0 else 0
        feat_cnl = in_cnl - width(in_embed) - embed - width(spatial_embed)
        if feat_cnl < 0 or (kernel_type == "DSK" and feat_cnl):
            raise L.EvdError(f"SparseBlurKernel.from_state_dict: row width {in_cnl} does not fit in_embed {in_embed}, embedding {embed}, spatial_embed {spatial_embed}")
        mod = cls(num_img, num_pt, kernel_hwindow, kernel_type, random_hwindow=random_hwindow, in_embed=in_embed, random_mode=random_mode,
                  view_embed_cnl=embed, spatial_embed=spatial_embed, num_hidden=num_hidden, num_wide=num_wide, feat_cnl=feat_cnl if kernel_type == "PBE" else 15,
                  short_cut=sd["linears1.0.weight"].shape[1] > num_wide, isglobal=isglobal, optim_trans="pattern_trans" in sd,
                  optim_spatialvariant_trans=sd["linears1.2.weight"].shape[0] == 5, poses=sd.get("poses"), view_embed=mlp)
        mod.load_state_dict(sd)
        return mod

    def _net(self):
        lins = [m for m in self.linears if isinstance(m, nn.Linear)] + [self.linears1[0], self.linears1[2]]
        return tuple(t for m in lins for t in (m.weight, m.bias))

    def _desc(self, H, W, K, Cw, n_img):
        return L.SparseBlurDesc(kernel_type=int(self.kernel_type == "PBE"), num_pt=self.num_pt, in_embed=self.in_embed, spatial_embed=self.spatial_embed,
                                embed_cnl=Cw, feat_cnl=self.feat_cnl if self.kernel_type == "PBE" else 0, num_hidden=self.num_hidden, num_wide=self.num_wide,
                                short_cut=int(bool(self.short_cut)), isglobal=int(bool(self.isglobal)), optim_trans=int(bool(self.optim_trans)),
                                optim_spatialvariant_trans=int(bool(self.optim_sv_trans)), n_img=n_img, n_pattern=self.pattern_pos.shape[0],
                                poses_per_image=0 if self.poses is None else self.poses.shape[0], H=int(H), W=int(W),
                                kernel_hwindow=float(self.kernel_hwindow), random_hwindow=float(self.random_hwindow), fx=float(K[0][0]), fy=float(K[1][1]),
                                cx=float(K[0][2]), cy=float(K[1][2]))

    def forward(self, H, W, K, rays, rays_info, feats=None, return_img_embed=False, noise=None, **kwargs):
        if self.random_hwindow > 0 and self.random_mode == "output":
            raise NotImplementedError(f"{self.random_mode} for self.random_mode is not implemented")
        ids = rays_info["images_idx"].reshape(-1).to(torch.int64).contiguous()
        R, dev = ids.shape[0], ids.device
        flat = lambda a: a.reshape(-1).float().contiguous()
        rays_x, rays_y = flat(rays_info["rays_x"]), flat(rays_info["rays_y"])
        poses = (rays_info["poses"].float() if self.poses is None else self.poses).contiguous()
        if self.random_hwindow > 0:
            noise = torch.randn((R, self.num_pt, 2), device=dev) if noise is None else noise.reshape(R, self.num_pt, 2).float().contiguous()
        else:
            noise = None
        if self.kernel_type == "PBE" and feats is not None:
            feats = feats.reshape(R * self.num_pt, self.feat_cnl).float().contiguous()
        else:
            feats = None
        trans = self.pattern_trans if self.optim_trans else None
        if type(self.img_embed) in (ViewEmbedding, ViewEmbeddingMLP):
            table = _feature_table(self.img_embed)
            out = _SparseBlurFn.apply(self._desc(H, W, K, table.shape[1], table.shape[0]), ids, None, rays_x, rays_y, poses, noise, feats, self.pattern_pos,
                                      trans, table, *self._net())
            new_rays, weight, align, img_embed = out
        else:
            x = self.img_embed(ids).float().contiguous()
            new_rays, weight, align, _ = _SparseBlurFn.apply(self._desc(H, W, K, x.shape[1], 0), ids, x, rays_x, rays_y, poses, noise, feats, self.pattern_pos,
                                                             trans, None, *self._net())
            img_embed = x
        return new_rays, weight, (None if align is None else align.reshape(())), ({"img_embed": img_embed} if return_img_embed else {})
