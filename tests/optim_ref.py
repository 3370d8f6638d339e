"""Float64 numpy restatement of the optimizer step of run_nerf.py:593-613: torch.nn.utils.clip_grad_norm_ (norm type 2), the step of
torch.optim.Adam(amsgrad=False, maximize=False) as torch/optim/adam.py `_single_tensor_adam` writes it, and the learning-rate schedule.
The reference of tests/test_gpu_optim.py; itself pinned to torch in float64 by tests/test_optim_ref.py."""
import numpy as np


def lr_at(initial_lr, global_step, lrate_decay, warmup_iters=-1, warmup_factor=0.1):
    """run_nerf.py:603-613"""
    if warmup_iters > 0 and global_step < warmup_iters:
        scale = (1 - warmup_factor) * global_step / warmup_iters + warmup_factor
        return initial_lr * scale
    decay_rate = 0.1
    decay_steps = lrate_decay * 1000
    return initial_lr * (decay_rate ** (global_step / decay_steps))


def total_norm(grads):
    """L2 norm over every element of the gradients that exist"""
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """clip_grad_norm_: min(1, max_norm / (total_norm + 1e-6)); a NaN norm gives NaN"""
    c = max_norm / (norm + 1e-6)
    return 1.0 if c > 1.0 else c


class Adam:
    """params: list of float64 arrays (updated in place); group_of[i]: index into groups; groups: dicts with lr, betas, eps, weight_decay.
    The state is per parameter (step, exp_avg, exp_avg_sq), created by the first step that has a gradient for it."""

    def __init__(self, params, group_of, groups):
        self.params = [np.array(p, dtype=np.float64) for p in params]
        self.group_of, self.groups = list(group_of), groups
        self.step_count = [0] * len(params)
        self.exp_avg = [np.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [np.zeros_like(p) for p in self.params]

    def step(self, grads, max_norm=None, clip=None, coef=None):
        """grads[i] None: the parameter is skipped (state and step count untouched).  max_norm: the gradients of the parameters with
        clip[i] (default all) are scaled by the clip coefficient of their joint norm -- or by `coef`, where the caller has the
        coefficient an implementation formed in float32 and wants the element arithmetic alone.  Returns the norm (None without max_norm)."""
        clip = [True] * len(self.params) if clip is None else clip
        norm = None
        if max_norm is not None:
            norm = total_norm([g for g, c in zip(grads, clip) if c])
            coef = clip_coef(norm, max_norm) if coef is None else coef
        for i, g in enumerate(grads):
            if g is None:
                continue
            h = self.groups[self.group_of[i]]
            b1, b2 = h["betas"]
            g = np.asarray(g, np.float64)
            if max_norm is not None and clip[i]:
                g = g * coef
            p, m, v = self.params[i], self.exp_avg[i], self.exp_avg_sq[i]
            self.step_count[i] += 1
            t = self.step_count[i]
            if h["weight_decay"] != 0:
                g = g + h["weight_decay"] * p
            m += (1 - b1) * (g - m)
            v *= b2
            v += (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            denom = np.sqrt(v) / np.sqrt(bc2) + h["eps"]
            p -= (h["lr"] / bc1) * m / denom
        return norm
