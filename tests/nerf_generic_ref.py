"""float64 torch restatement of NeRF.mlpforward + eval (networks/nerf.py:46-72,131-162, embedding.py:88-98) for any depth, width,
frequency counts and skip index, and the cases of the generic training path's tests (tests/test_gpu_nerf_generic_train.py).  The
restatement returns the pre-activation of every ReLU; it is pinned to the reference's real NeRF class by golden G40
(tools/gen_golden_nerf_generic.py, tests/test_nerf_generic_ref.py).  The same class, through optional arguments that leave the plain
call untouched, is the reference of the inference pass's arm tests (tests/nerf_level_ref.py): the half-precision mode model, structural
faults, the two feature outputs and the use_viewdirs=False head.  Test infrastructure only."""
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


QUANT = {"f16": torch.float16, "bf16": torch.bfloat16}


def live_units(h):
    """indices of the units of a post-ReLU activation [n, W] that are positive on at least a quarter of the samples, ascending"""
    return torch.nonzero((h > 0).double().mean(0) >= 0.25).reshape(-1).tolist()


def swap_pair(h):
    """two live units of one 16-block whose activations differ, highest-indexed first; None if there are none"""
    live = live_units(h)
    for u in reversed(live):
        for v in reversed(live):
            if v < u and v // 16 == u // 16 and not torch.equal(h[:, u], h[:, v]):
                return u, v
    return None


class GenericNerf(torch.nn.Module):
    """NeRF.eval on embedded inputs, networks/nerf.py:131-162: D layers of width W, `skip` = the one index of `skips` (None: no skip; the
    reference concatenates AFTER layer `skip`, so the next layer is the wide one).  use_viewdirs=False: `output_linear` replaces the view
    branch (nerf.py:158-160), raw = its rows 0..3, dirs is not read.

    forward() alone is the exact float64 network.  Its optional arguments serve tests/nerf_level_ref.py:
      quant   "f16" / "bf16", the MODEL of the single-product half-precision modes: weights rounded to nearest in the type, the input of
              every linear layer (both encodings, hidden activations after ReLU, the feature_linear output entering views_linears.0, the
              views activation entering rgb_linear) rounded to nearest in the type, products and sums exact, biases float32 values added
              in float64; raw and the feature rows that are OUTPUT are left unrounded.
      fault   one structural fault, what a packing or column-map mistake produces (nerf_level_ref.faults_of lists those of a network).
              A fault on a unit picks the highest-indexed live unit (live_units) of that activation, on this call's own samples.
      out     a dict that receives "feature1" (the feature_linear output, extract_feature="after_linear"; None without the view branch),
              "feature2" (h after the last pts_linears ReLU, "before_linear"; always [n, W]: a skip index of D-1 never concatenates),
              "A" (the largest absolute output of any linear layer) and "unit" (what a unit fault picked, None where nothing was live)."""

    def __init__(self, sd, D, Wd, L, Lv, skip, prefix="", use_viewdirs=True):
        super().__init__()
        self.D, self.W, self.L, self.Lv, self.skip, self.use_viewdirs = D, Wd, L, Lv, skip, use_viewdirs
        self.p = torch.nn.ParameterDict({k[len(prefix):].replace(".", "_"): torch.nn.Parameter(torch.tensor(np.asarray(v), dtype=torch.float64))
                                         for k, v in sd.items() if k.startswith(prefix)})

    def lin(self, name, x, quant=None, fault=None, rec=None):
        w = self.p[name + "_weight"]
        if quant is not None:
            x, w = x.to(QUANT[quant]).double(), w.to(QUANT[quant]).double()
        y = x @ w.T
        if name + "_bias" in self.p and fault != "nobias_" + name:
            y = y + self.p[name + "_bias"]
        if rec is not None:
            rec.append(float(y.detach().abs().max()))
        return y

    @staticmethod
    def _without(x, cols):
        x = x.clone()
        x[:, cols] = 0
        return x

    def _unit_fault(self, h, kind, out):
        """hid: zero the highest-indexed live unit; swap: exchange two live units of one 16-block"""
        if kind == "hid":
            live = live_units(h)
            pick = live[-1] if live else None
            if pick is not None:
                h = self._without(h, [pick])
        else:
            pick = swap_pair(h)
            if pick is not None:
                h = h.clone()
                h[:, list(pick)] = h[:, list(pick[::-1])]
        if out is not None:
            out["unit"] = pick
        return h

    def forward(self, pts, dirs, pre=None, quant=None, fault=None, out=None):
        """raw [n, 4] = (rgb, alpha); pre: dict that receives the pre-activation of every ReLU ("h0" .. "h{D-1}", "hv")"""
        rec = [] if out is not None else None
        lin = lambda name, x: self.lin(name, x, quant, fault.replace(".", "_") if fault else None, rec)     # "nobias_views_linears.0"
        pe = embed(pts, self.L)
        pe0 = self._without(pe, [-3, -2, -1]) if fault == "top_pts_cos" else pe
        pe_skip = self._without(pe, [-3, -2, -1]) if fault == "skip_top_cos" else pe
        h = pe0
        for l in range(self.D):
            x = lin(f"pts_linears_{l}", h)
            if pre is not None:
                pre[f"h{l}"] = x
            h = torch.relu(x)
            if fault in (f"hid{l}", f"swap{l}"):
                h = self._unit_fault(h, fault[:-len(str(l))], out)
            if self.skip is not None and l == self.skip and l < self.D - 1:
                h = torch.cat([pe_skip, h], -1)
        if out is not None:
            out["feature2"] = torch.roll(h, 1, 1) if fault == "feat_roll" else h
        if not self.use_viewdirs:
            raw = lin("output_linear", h)[:, :4]
            if fault == "out_swap":
                raw = raw[:, [0, 1, 3, 2]]
            if out is not None:
                out["feature1"], out["A"] = None, max(rec)
            return raw
        ped = embed(dirs, self.Lv)
        if fault == "top_dir_cos":
            ped = self._without(ped, [-3, -2, -1])
        alpha = lin("alpha_linear", h)
        f = lin("feature_linear", h)
        if out is not None:
            out["feature1"] = torch.roll(f, 1, 1) if fault == "feat_roll" else f
        x = lin("views_linears_0", torch.cat([self._without(f, [-1]) if fault == "last_feat" else f, ped], -1))
        if pre is not None:
            pre["hv"] = x
        hv = torch.relu(x)
        if fault == "last_hv":
            hv = self._unit_fault(hv, "hid", out)
        raw = torch.cat([lin("rgb_linear", hv), alpha], -1)
        if out is not None:
            out["A"] = max(rec)
        return raw


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
