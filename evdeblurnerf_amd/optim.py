"""The optimizer step of the reference's training iteration (run_nerf.py:593-613) on libevdnerf.so: clip_grad_norm_, the step of
torch.optim.Adam over the reference's parameter groups, and the learning-rate schedule.

`Adam` is a torch.optim.Optimizer whose step() is ONE launch over every parameter (evd_adam_step, csrc/kernels_optim.hip).  Given the
model, the same pass writes the new grid values into the PDRF levels' own float32 / float16 copies (so the next forward reloads
nothing), can clear the gradients of the in-place mode, and tells the model exactly what changed.  Its state dict interchanges with
torch.optim.Adam's.  There is no PyTorch fall-back: without the library this module raises."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def lr_at(initial_lr, global_step, lrate_decay, warmup_iters=-1, warmup_factor=0.1):
    """run_nerf.py:603-613: the learning rate the reference assigns to a group AFTER the optimizer step of iteration `global_step`
    (lrate_decay in thousands of steps)."""
    if warmup_iters > 0 and global_step < warmup_iters:
        return initial_lr * ((1 - warmup_factor) * global_step / warmup_iters + warmup_factor)
    return initial_lr * (0.1 ** (global_step / (lrate_decay * 1000)))


def _check_tensor(t, what):
    if not isinstance(t, torch.Tensor):
        raise L.EvdError(f"{what}: not a tensor")
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.is_sparse):
        raise L.EvdError(f"{what}: the device step takes contiguous float32 CUDA tensors, got "
                         f"{tuple(t.shape)} {t.dtype} on {t.device}" + ("" if t.is_contiguous() else " (not contiguous)"))


class _Segments:
    """An evd_adam handle over a fixed list of (parameter, exp_avg, exp_avg_sq, mirrors) arrays, with its device scratch"""

    def __init__(self, rows, ngroups, device):
        """rows: [(param ptr, exp_avg ptr, exp_avg_sq ptr, mirror_f32 ptr | None, mirror_f16 ptr | None, n, group, clip)]"""
        self.n = len(rows)
        segs = (L.AdamSegment * max(self.n, 1))()
        for s, (p, m, v, f32, f16, n, group, clip) in zip(segs, rows):
            s.param, s.exp_avg, s.exp_avg_sq, s.mirror_f32, s.mirror_f16, s.n, s.group, s.clip = p, m, v, f32, f16, n, group, int(clip)
        h = C.c_void_p()
        L.check(L.lib().evd_adam_create(segs, self.n, ngroups, C.byref(h)), "evd_adam_create")
        self._h = h
        self.nbytes = int(L.lib().evd_adam_workspace_bytes(h))
        self.ws = torch.empty((self.nbytes,), dtype=torch.uint8, device=device)
        self.grads = (C.c_void_p * max(self.n, 1))()
        self.norm = torch.zeros((1,), dtype=torch.float32, device=device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and L is not None and getattr(L, "lib", None) is not None:
            L.lib().evd_adam_destroy(h)
            self._h = None

    def grad_norm(self):
        L.check(L.lib().evd_grad_norm(self._h, self.grads, L.ptr(self.norm), L.ptr(self.ws), self.nbytes, L.stream_ptr()), "evd_grad_norm")
        return self.norm


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(amsgrad=False, maximize=False) with the step on the device in one launch.

    params_or_groups, lr, betas, eps, weight_decay: as torch.optim.Adam (per-group overrides, extra keys such as `initial_lr` are
    kept; `param_groups[i]["lr"]` may be reassigned between steps).  Every parameter is a contiguous float32 CUDA tensor.
    model: a NeRFAll in training mode.  Its grid tensors are then also written into the levels' own copies by the step (the level
      is told so and reloads nothing), and its networks' packed streams are marked stale.  None: nothing is mirrored or marked; the
      library reloads because a backward ran, as it does after torch's fused Adam.
    max_grad_norm: clip_grad_norm_(clip_params, max_grad_norm) folded into the step (the norm is one more launch pair; the stored
      gradients are not rescaled); clip_params defaults to the model's parameters, without a model to all of the optimizer's.
    zero_grads: the step clears every gradient it consumed; `.grad` stays attached.  With a model this needs
      enable_training(grads_in_place=True): the next backward then adds into the kept buffers without a fill."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0., model=None, max_grad_norm=None, clip_params=None,
                 zero_grads=False):
        if not (lr >= 0 and eps >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and weight_decay >= 0):
            raise ValueError(f"invalid Adam hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        L.lib()
        # the keys torch.optim.Adam keeps in a group, so that a state dict loads into either class
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self.model, self.max_grad_norm, self.zero_grads = model, max_grad_norm, bool(zero_grads)
        if model is not None:
            model._require_training()
            if self.zero_grads and not getattr(model, "_grads_in_place", False):
                raise L.EvdError("zero_grads=True needs the model's in-place gradient buffers: enable_training(..., grads_in_place=True)")
        if clip_params is None:
            clip_params = model.parameters() if model is not None else [p for g in self.param_groups for p in g["params"]]
        self._clip_ids = {id(p) for p in clip_params}
        self.total_norm = None              # device scalar of the last clipped step
        self._seg = None
        self._key = None

    # ---- the segment table: rebuilt when the set of parameters or their storage changes (add_param_group, load_state_dict)
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _table_key(self):
        return tuple(p.data_ptr() for g in self.param_groups for p in g["params"]) + tuple(len(g["params"]) for g in self.param_groups)

    def _mirrors(self):
        out = {}
        if self.model is None:
            return out
        self._levels = []
        for lv in self.model._levels:
            if lv is None or lv.grids is None:
                continue
            grids = list(lv.grids.values())
            f32, f16 = lv.net.grid_mirrors()
            sizes = (C.c_long * 7)()
            L.check(L.lib().evd_voxel_grid_sizes(lv.net.handle, sizes), "evd_voxel_grid_sizes")
            for t, n, a, b in zip(grids, sizes, f32, f16):
                if t.numel() != n:
                    raise L.EvdError(f"grid tensor of {t.numel()} elements, the level keeps {n}")
                out[id(t)] = (a, b)
            self._levels.append((lv.net, grids))
        return out

    def _build(self):
        params = self._params()
        if not params:
            raise L.EvdError("optim.Adam: no parameters")
        dev = params[0].device
        for p in params:
            _check_tensor(p, "optim.Adam parameter")
            if p.device != dev:
                raise L.EvdError("optim.Adam: all parameters on one device")
        mirrors = self._mirrors()
        # flat moment buffers; every parameter's slot starts at its own phase within 16 bytes, so the step moves 16-byte vectors
        offs, total = [], 0
        for p in params:
            phase = (p.data_ptr() % 16) // 4
            offs.append(total + phase)
            total += -(-(phase + p.numel()) // 4) * 4
        self._exp_avg = torch.zeros((total,), dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros((total,), dtype=torch.float32, device=dev)
        self._steps_t = torch.zeros((len(params),), dtype=torch.float32)            # the `step` entries of the state are views of it
        self._steps = self._steps_t.numpy()
        self._steps_c = np.zeros((len(params),), dtype=np.int64)
        self._views, self._has_state, rows = [], [], []
        gi = {id(p): k for k, g in enumerate(self.param_groups) for p in g["params"]}
        for i, (p, o) in enumerate(zip(params, offs)):
            n = p.numel()
            m, v = self._exp_avg[o:o + n].view(p.shape), self._exp_avg_sq[o:o + n].view(p.shape)
            old = self.state.get(p)
            if old:                         # state that exists already (torch's, or this class's before a rebuild) moves into the flat buffers
                m.copy_(old["exp_avg"])
                v.copy_(old["exp_avg_sq"])
                self._steps[i] = float(old["step"])
                self.state[p] = {"step": self._steps_t[i], "exp_avg": m, "exp_avg_sq": v}
            self._views.append((m, v))
            self._has_state.append(bool(old))
            f32, f16 = mirrors.get(id(p), (None, None))
            rows.append((p.data_ptr(), m.data_ptr(), v.data_ptr(), f32, f16, n, gi[id(p)], id(p) in self._clip_ids))
        self._seg = _Segments(rows, len(self.param_groups), dev)
        self._plist = params
        self._pos = {id(p): i for i, p in enumerate(params) if id(p) in mirrors}
        self._groups_c = (L.AdamGroup * len(self.param_groups))()
        self._key = self._table_key()

    def add_param_group(self, group):
        super().add_param_group(group)
        self._key = None

    def load_state_dict(self, state_dict):
        """accepts torch.optim.Adam's state dict (and this class's): the moments are copied into the flat buffers"""
        for g in state_dict["param_groups"]:
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
                raise L.EvdError("optim.Adam: amsgrad / maximize / decoupled weight decay are not built")
        super().load_state_dict(state_dict)
        self._key = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._key is None or self._key != self._table_key():
            self._build()
        seg, grads = self._seg, self._seg.grads
        stepped = np.zeros((seg.n,), dtype=bool)
        for i, p in enumerate(self._plist):
            g = p.grad
            if g is None:
                grads[i] = None
                continue
            if not (g.dtype == torch.float32 and g.is_contiguous() and g.is_cuda and not g.is_sparse):
                raise L.EvdError(f"optim.Adam: gradient of parameter {i} is not a contiguous float32 CUDA tensor")
            grads[i] = g.data_ptr()
            stepped[i] = True
            if not self._has_state[i]:
                m, v = self._views[i]
                self.state[p] = {"step": self._steps_t[i], "exp_avg": m, "exp_avg_sq": v}
                self._has_state[i] = True
        for gc, g in zip(self._groups_c, self.param_groups):
            gc.lr, (gc.beta1, gc.beta2), gc.eps, gc.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        max_norm = 0.
        if self.max_grad_norm is not None:
            self.total_norm = seg.grad_norm()
            max_norm = float(self.max_grad_norm)
        self._steps_c[:] = self._steps
        L.check(L.lib().evd_adam_step(seg._h, grads, self._steps_c.ctypes.data_as(C.POINTER(C.c_long)), self._groups_c, len(self.param_groups),
                                      max_norm, L.ptr(self.total_norm) if max_norm > 0 else None, int(self.zero_grads), L.ptr(seg.ws), seg.nbytes,
                                      L.stream_ptr()), "evd_adam_step")
        self._steps[stepped] += 1
        if self.model is not None:
            self.model.invalidate_packed()          # the networks' streams are re-packed by the next forward (the re-pack itself is unchanged)
            for net, grids in self._levels:         # a level whose seven grids all went through the mirrors holds the current values
                if all(id(t) in self._pos and stepped[self._pos[id(t)]] for t in grids):
                    net.grids_loaded(grids)
        return loss


_NORM_CACHE = {}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=2) for loops that clip outside the step: the norm is evd_grad_norm
    (float64 partial sums in a fixed order: the same bits from call to call), the scale an in-place multiply of the gradients by
    min(1, max_norm / (norm + 1e-6)).  Returns the total norm as a device tensor; nothing synchronises."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.)
    for g in grads:
        _check_tensor(g, "clip_grad_norm_ gradient")
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    seg = _NORM_CACHE.get(key)
    if seg is None:
        if len(_NORM_CACHE) >= 4:           # the gradient buffers of a training loop are persistent: a handful of tables is plenty
            _NORM_CACHE.pop(next(iter(_NORM_CACHE)))
        # the norm reads the gradients only: they stand in for the table's parameter / moment columns, which give the 16-byte framing
        seg = _Segments([(a, a, a, None, None, n, 0, True) for a, n in key], 1, grads[0].device)
        for i, (a, _) in enumerate(key):
            seg.grads[i] = a
        _NORM_CACHE[key] = seg
    total = seg.grad_norm().clone()[0]
    coef = torch.clamp(float(max_norm) / (total + 1e-6), max=1.0)
    torch._foreach_mul_(grads, coef)
    return total
