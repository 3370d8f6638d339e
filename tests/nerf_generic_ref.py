"""float64 torch restatement of NeRF.mlpforward + eval (networks/nerf.py:46-72,131-162, embedding.py:88-98) for any depth, width,
frequency counts and skip index, and the cases of the generic training path's tests (tests/test_gpu_nerf_generic_train.py).  The
restatement returns the pre-activation of every ReLU; it is pinned to the reference's real NeRF class by golden G40
(tools/gen_golden_nerf_generic.py, tests/test_nerf_generic_ref.py).  Test infrastructure only."""
import functools

import numpy as np
import torch

from evdeblurnerf_amd import weights as W
from test_gpu_train import make_inputs
from torch_restatement import embed

# name: (D, W, L, Lv, skip or None, R, S, scale of d raw)
CASES = {
    "a": (4, 64, 6, 2, None, 37, 9, 3.0),         # partial tile, G24's small shape
    "b": (3, 128, 10, 4, 0, 64, 33, 1e-4),        # new width, skip at the first layer
    "c": (8, 256, 6, 2, 4, 48, 40, 1e-2),         # the shipped shape with other frequency counts
    "d": (6, 64, 3, 8, 2, 70, 19, 1e-9),          # four direction k-steps, several workgroups
    "e": (1, 64, 0, 0, None, 3, 5, 1.0),          # one layer, no frequencies, under one tile
    "f": (2, 256, 10, 10, 0, 40, 16, 1e-2),       # skip feeding the last layer, widest encodings
}
TAU = 2e-6          # a sample with a float64 pre-activation inside (-TAU, TAU) gets d raw = 0: its ReLU is decided by rounding
TIE_CAP = 0.10      # at most this fraction of a case's samples may be zeroed


def case_state_dict(name):
    D, Wd, L, Lv, skip, _, _, _ = CASES[name]
    return W.make_nerf_state_dict(400 + ord(name), D, Wd, input_ch=W.pe_dim(L), input_ch_views=W.pe_dim(Lv),
                                  skips=() if skip is None else (skip,))


def case_inputs(name):
    """ray batch [R, 11], z [R, S], d raw [R, S, 4] (tests/test_gpu_train_f32grade.py:40-41), all float32"""
    _, _, _, _, _, R, S, gscale = CASES[name]
    rb, z = make_inputs(R, S, 6)
    rs = np.random.RandomState(9)
    d_raw = (rs.normal(size=(R, S, 4)) * gscale * np.exp(rs.uniform(-4, 0, (R, S, 1)))).astype(np.float32)
    return rb, z, d_raw


def positions(rb, z):
    """float64 copies of the FLOAT32 sample positions pts = o + d z (renderer.py:180) and of the per-sample view directions"""
    S = z.shape[1]
    pts = torch.tensor(rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None], dtype=torch.float64).reshape(-1, 3)
    dirs = torch.tensor(np.repeat(rb[:, None, 8:11], S, 1), dtype=torch.float64).reshape(-1, 3)
    return pts, dirs


class GenericNerf(torch.nn.Module):
    """NeRF.eval on embedded inputs, networks/nerf.py:131-162 with use_viewdirs: D layers of width W, `skip` = the one index of
    `skips` (None: no skip; the reference concatenates AFTER layer `skip`, so the next layer is the wide one)"""

    def __init__(self, sd, D, Wd, L, Lv, skip, prefix=""):
        super().__init__()
        self.D, self.W, self.L, self.Lv, self.skip = D, Wd, L, Lv, skip
        self.p = torch.nn.ParameterDict({k[len(prefix):].replace(".", "_"): torch.nn.Parameter(torch.tensor(np.asarray(v), dtype=torch.float64))
                                         for k, v in sd.items() if k.startswith(prefix)})

    def lin(self, name, x):
        y = x @ self.p[name + "_weight"].T
        return y + self.p[name + "_bias"] if name + "_bias" in self.p else y

    def forward(self, pts, dirs, pre=None):
        """raw [n, 4] = (rgb, alpha); pre: dict that receives the pre-activation of every ReLU ("h0" .. "h{D-1}", "hv")"""
        pe, ped = embed(pts, self.L), embed(dirs, self.Lv)
        h = pe
        for l in range(self.D):
            x = self.lin(f"pts_linears_{l}", h)
            if pre is not None:
                pre[f"h{l}"] = x
            h = torch.relu(x)
            if self.skip is not None and l == self.skip and l < self.D - 1:
                h = torch.cat([pe, h], -1)
        alpha = self.lin("alpha_linear", h)
        f = self.lin("feature_linear", h)
        x = self.lin("views_linears_0", torch.cat([f, ped], -1))
        if pre is not None:
            pre["hv"] = x
        return torch.cat([self.lin("rgb_linear", torch.relu(x)), alpha], -1)


def case_net(name, sd=None):
    D, Wd, L, Lv, skip, _, _, _ = CASES[name]
    return GenericNerf(sd if sd is not None else case_state_dict(name), D, Wd, L, Lv, skip)


def tie_samples(pre, tau=TAU):
    """[n] bool: samples with a pre-activation inside (-tau, tau)"""
    return torch.stack([(v.detach().abs() < tau).any(-1) for v in pre.values()]).any(0)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """Computed once per session and shared: (raw [n, 4] float64, {state-dict key: float64 gradient}, d raw [R, S, 4] float32 with the tie
    samples zeroed, fraction of samples zeroed).  The gradients are those of sum(raw * d raw) with the zeroed d raw."""
    rb, z, d_raw = case_inputs(name)
    net = case_net(name)
    pts, dirs = positions(rb, z)
    pre = {}
    raw = net(pts, dirs, pre)
    ties = tie_samples(pre)
    d_raw = d_raw.copy()
    d_raw.reshape(-1, 4)[ties.numpy()] = 0.0
    (raw * torch.tensor(d_raw, dtype=torch.float64).reshape(-1, 4)).sum().backward()
    grads = {k: net.p[k.replace(".", "_")].grad.clone() for k in case_state_dict(name)}
    return raw.detach(), grads, d_raw, float(ties.double().mean().item())
