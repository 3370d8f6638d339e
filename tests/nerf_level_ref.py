"""float64 reference of the inference pass of one NeRF level (NeRF.mlpforward + eval, networks/nerf.py:46-72,131-162), the model of the
single-product half-precision modes, the bound every output of evd_nerf_mlp is held to, the structural faults that keep those bounds
honest, and the case matrix of tests/test_gpu_nerf_level_forward.py.  Test infrastructure only; nothing here needs a GPU
(tests/test_nerf_level_ref.py).

The network is nerf_generic_ref.GenericNerf (pinned to the reference's NeRF class by golden G40) with its optional arguments: quant (the
mode model), fault, the two feature outputs, use_viewdirs=False.  Its output_linear head is pinned to the oracle in the CPU test.

Weights.  weights.make_nerf_state_dict draws U(+-1/sqrt(fan_in)); a stack of such layers contracts, and a mistake in an early layer moves
raw by less than any bound (on the 8 x 256 network a dead unit after layer 3 moves raw by 3.5e-6).  So every network here has its
pts_linears.*.weight scaled by a gain (NETS: seed and gain per network, chosen on the CPU until every fault of faults_of() exceeds the
bounds by the factors tests/test_nerf_level_ref.py asserts, with the largest pre-activation A kept below 8).

bounds            bound(X) = 4 E_q(X) + F for X in {raw, feature}, from the two float64 evaluations alone:
                  E_q(X)   L-inf distance of the quantised model's X from the exact one (0 in the float32-grade modes f32, f16x3, f16c);
                           4 = 2 (a kernel that truncates where the model rounds to nearest) x 2 (float32 accumulation, and a finite
                           sample under-reading the worst case);
                  F        5e-5 max(1, A), voxel_level_ref.F32_GRADE: the project's float32-grade figure for these networks on raw
                           against float64, A the largest absolute output of a linear layer of the float64 network in the case.
Nothing measured on a kernel enters a bound.

CASES is the arm matrix: every case names the arm of evd_nerf_mlp (csrc/evd_api.hip) it reaches, and expected_arm() re-derives that arm
from the case's construction alone, mirroring evd_nerf_create and evd_nerf_mlp.  Sizes R x S: 1 x 1; 3 x 43 = 129 (one sample past the
128-sample workgroup of f32 / f16x3 and the f16c tile); 37 x 7 = 259 (three past the 256 of bf16 / f16); 70 x 33 = 2310 (many workgroups,
a ragged last one); and for f16c R = None: (CUs + 1) x 128, one 128-sample tile more than the persistent grid has workgroups (rows())."""
import functools

import numpy as np
import torch

import nerf_generic_ref as G
from evdeblurnerf_amd import weights as W
from voxel_level_ref import F32_GRADE

QUANT = G.QUANT
MODES = ("f32", "f16x3", "f16", "bf16")
HALF = ("bf16", "f16", "f16x3")             # the modes the pipelined kernel is built in
# what a fault's change must be of the bound it is compared with, by mode (tests/test_nerf_level_ref.py); bf16: strictly above
VISIBLE = {"f32": 10.0, "f16x3": 10.0, "f16c": 10.0, "f16": 2.0, "bf16": 1.0}
# (network, R, S, kind, fault) whose change stays at or below the bf16 bound; at most a tenth of the bf16 pairs, and every fault is still
# visible in bf16 in some case of each bf16 arm that has it
BF16_BLIND = (("c", 3, 43, 0, "hid4"), ("c", 37, 7, 0, "hid4"), ("c", 70, 33, 1, "last_feat"),      # ratios 0.99, 0.87, 0.97
              ("deep", 37, 7, 0, "hid6"), ("deep", 37, 7, 0, "last_feat"))                                # 0.58, 0.86: 5 of 835 pairs

# network: D, W, multires, multires_views, skip or None, weight seed, gain on pts_linears.*.weight, output_ch (0: the view branch)
NETS = {
    "std": (8, 256, 10, 4, 4, 409, 1.9, 0),            # the shipped shape: the one network with pipelined and f16c kernels
    "a": (4, 64, 6, 2, None, 497, 1.7, 0),             # the six shapes of nerf_generic_ref.CASES, with its seeds
    "b": (3, 128, 10, 4, 0, 498, 2.0, 0),
    "c": (8, 256, 6, 2, 4, 529, 1.9, 0),
    "d": (6, 64, 3, 8, 2, 520, 2.0, 0),
    "e": (1, 64, 0, 0, None, 501, 1.7, 0),
    "f": (2, 256, 10, 10, 0, 532, 1.7, 0),
    "deep": (14, 256, 10, 4, 7, 417, 2.1, 0),          # 14 x 256 + 448 = 4032 bias floats of the 4096 the LDS block holds; D = 15 is refused
    "nv256o4": (8, 256, 10, 4, 4, 65, 2.0, 4),         # use_viewdirs=False: output_linear with 4 and 5 rows
    "nv256o5": (8, 256, 10, 4, 4, 62, 2.0, 5),
    "nv64o4": (4, 64, 6, 4, 1, 63, 1.8, 4),
    "nv64o5": (4, 64, 6, 4, 1, 64, 1.8, 5),
}
SIZES = ((1, 1), (3, 43), (37, 7), (70, 33))
WG = {"bf16": 256, "f16": 256, "f32": 128, "f16x3": 128, "f16c": 128}     # samples per workgroup (per tile in f16c)


def net_dims(net):
    D, Wd, L, Lv, skip, _, _, och = NETS[net]
    return D, Wd, L, Lv, skip, och


@functools.lru_cache(maxsize=None)
def state_dict(net, rgb_bias=True):
    """make_nerf_state_dict of the network's seed with the gain applied to pts_linears.*.weight (float32); shared, do not write"""
    D, Wd, L, Lv, skip, seed, gain, och = NETS[net]
    sd = W.make_nerf_state_dict(seed, D, Wd, input_ch=W.pe_dim(L), input_ch_views=W.pe_dim(Lv) if not och else 0,
                                skips=() if skip is None else (skip,), use_viewdirs=not och, rgb_add_bias=rgb_bias, output_ch=och or 4)
    for l in range(D):
        sd[f"pts_linears.{l}.weight"] = (sd[f"pts_linears.{l}.weight"] * np.float32(gain)).astype(np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def _model(net, rgb_bias, dev):
    D, Wd, L, Lv, skip, och = net_dims(net)
    return G.GenericNerf(state_dict(net, rgb_bias), D, Wd, L, Lv, skip, use_viewdirs=not och).to(dev)


@functools.lru_cache(maxsize=None)
def inputs(R, S, ncol=11):
    """float32 ray batch [R, ncol] (o in +-0.5, unit d, near 0, far 1, and with 11 columns viewdirs = d) and sorted z [R, S] in (0.2, 2)"""
    rs = np.random.RandomState(11 + R + 1000 * S)
    rb = np.zeros((R, ncol), np.float32)
    rb[:, 0:3] = rs.uniform(-0.5, 0.5, (R, 3))
    d = rs.normal(size=(R, 3))
    rb[:, 3:6] = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rb[:, 7] = 1.0
    if ncol == 11:
        rb[:, 8:11] = rb[:, 3:6]
    return rb, np.sort(rs.uniform(0.2, 2.0, (R, S)).astype(np.float32), -1)


def faults_of(net, rgb_bias=True, kind=0):
    """the structural faults that apply to a network (and, for feat_roll, to a launch that outputs feature rows)"""
    D, Wd, L, Lv, skip, och = net_dims(net)
    f = ["top_pts_cos"] + (["skip_top_cos"] if skip is not None and skip < D - 1 else [])
    f += [f"{k}{l}" for l in range(D) for k in ("hid", "swap")] + [f"nobias_pts_linears.{l}" for l in range(D)]
    if och:
        f += ["nobias_output_linear", "out_swap"]
    else:
        f += ["top_dir_cos", "last_feat", "last_hv", "nobias_alpha_linear", "nobias_feature_linear", "nobias_views_linears.0"]
        f += ["nobias_rgb_linear"] if rgb_bias else []
    return tuple(f + (["feat_roll"] if kind else []))


def evaluate_net(net, R, S, rgb_bias=True, dev="cpu", quant=None, fault=None):
    """the float64 outputs of a network on inputs(R, S): dict(raw [n, 4], feature1 [n, W] | None, feature2 [n, W], A, unit)"""
    och = net_dims(net)[5]
    rb, z = inputs(R, S, 8 if och else 11)
    rb, z = torch.as_tensor(rb).to(dev), torch.as_tensor(z).to(dev)
    with torch.no_grad():
        pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).double().reshape(-1, 3)        # the float32 o + d z of renderer.py:180
        dirs = None if och else rb[:, None, 8:11].expand(R, S, 3).double().reshape(-1, 3)
        out = {}
        out["raw"] = _model(net, rgb_bias, str(dev))(pts, dirs, quant=quant, fault=fault, out=out)
    return out


# ---- the case matrix ---------------------------------------------------------------------------------------------------------------
def case(arm, net, mode, R, S, kind=0, rgb_bias=True, prefill=False):
    """kind: 0 no feature rows, 1 extract_feature="after_linear", 2 "before_linear".  prefill: run through a direct evd_nerf_mlp call on
    NaN-filled outputs instead of NeRF.mlpforward.  R = None: CUs + 1 rows (rows())"""
    cid = f"{arm}-{net}-{mode}-{'cus1' if R is None else R}x{S}" + (f"-kind{kind}" if kind else "") + ("" if rgb_bias else "-norgbbias")
    return dict(id=cid, arm=arm, net=net, mode=mode, R=R, S=S, kind=kind, rgb_bias=rgb_bias, prefill=prefill)


def rows(c, cus=256):
    return cus + 1 if c["R"] is None else c["R"]


def expected_arm(c):
    """the arm of evd_nerf_mlp a case reaches, from its construction (evd_nerf_create's streams and evd_nerf_mlp's dispatch restated);
    None: the call is refused"""
    D, Wd, L, Lv, skip, och = net_dims(c["net"])
    standard, no_views, feature = (L, Lv) == (10, 4), bool(och), c["kind"] != 0
    built = Wd == 256 and D == 8 and skip == 4              # nerf_pipe_built / nerf_c_built
    if no_views:
        return None if (c["mode"] == "f16c" or c["kind"] == 1) else "noviews"
    if c["mode"] == "f16c":
        return "c" if (standard and built and not feature) else None
    if standard and built and c["mode"] in HALF:
        return "pipe_feat" if feature else "pipe"
    return "generic_feat" if feature else "generic"


def _cases():
    out = []
    for R, S in SIZES + ((None, 128),):
        out.append(case("c", "std", "f16c", R, S, prefill=(R, S) == (3, 43)))
    out.append(case("c", "std", "f16c", 70, 33, rgb_bias=False))
    for m in HALF:
        for R, S in SIZES:
            out.append(case("pipe", "std", m, R, S, prefill=(R, S) == (37, 7)))
            out.append(case("pipe_feat", "std", m, R, S, kind=1, prefill=(R, S) == (37, 7)))
        for R, S in ((1, 1), (37, 7), (70, 33)):
            out.append(case("pipe_feat", "std", m, R, S, kind=2))
    for R, S in SIZES:
        out.append(case("generic", "std", "f32", R, S))
    for R, S in ((37, 7), (70, 33)):
        for kind in (1, 2):
            out.append(case("generic_feat", "std", "f32", R, S, kind=kind))
    # the six shapes: two sizes each without rows, one with; kinds so that D = 1 (e) and a wide last layer (f) have kind 2
    plain = {"a": ((3, 43), (70, 33)), "b": ((1, 1), (37, 7)), "c": ((3, 43), (37, 7)), "d": ((1, 1), (70, 33)), "e": ((3, 43), (37, 7)),
             "f": ((1, 1), (70, 33))}
    rows_ = (("a", 1, (37, 7)), ("b", 1, (70, 33)), ("b", 2, (1, 1)), ("c", 1, (70, 33)), ("c", 2, (3, 43)), ("d", 2, (37, 7)), ("e", 1, (70, 33)),
             ("e", 2, (37, 7)), ("f", 1, (3, 43)), ("f", 2, (70, 33)))
    for m in MODES:
        for net, sizes in plain.items():
            for R, S in sizes:
                out.append(case("generic", net, m, R, S, prefill=(net, R, m) == ("d", 70, "f16")))
        out.append(case("generic", "deep", m, 37, 7))
        for net, kind, (R, S) in rows_:
            out.append(case("generic_feat", net, m, R, S, kind=kind, prefill=(net, kind, m) == ("e", 2, "bf16")))
    out.append(case("generic_feat", "deep", "f16x3", 3, 43, kind=2))
    for m in MODES:
        for net, (sa, sb) in (("nv256o4", ((70, 33), (3, 43))), ("nv256o5", ((37, 7), (1, 1))), ("nv64o4", ((1, 1), (37, 7))),
                              ("nv64o5", ((3, 43), (70, 33)))):
            out.append(case("noviews", net, m, *sa, prefill=(net, m) == ("nv256o5", "f32")))
            out.append(case("noviews", net, m, *sb, kind=2, prefill=(net, m) == ("nv64o4", "f16x3")))
    return out


CASES = _cases()


def outputs_of(c, o):
    """what a case outputs of an evaluate_net() result"""
    return dict(raw=o["raw"], feature=o[f"feature{c['kind']}"] if c["kind"] else None, A=o["A"], unit=o.get("unit"))


def bound_of(exact, model, A):
    """4 E_q + F for one output; model: the quantised evaluation of that output, None in the float32-grade modes"""
    e_q = float((model - exact).abs().max()) if model is not None else 0.0
    return 4 * e_q + F32_GRADE * max(1.0, A), e_q


def bounds(c, exact, model=None):
    """exact, model: outputs_of() the float64 evaluation and (f16 / bf16 cases) the quantised one -> ({"raw" | "feature": bound}, {..: E_q}).
    Only the two float64 evaluations enter."""
    assert (model is not None) == (c["mode"] in QUANT)
    bound, e_q = {}, {}
    for k in ("raw", "feature"):
        if exact[k] is not None:
            bound[k], e_q[k] = bound_of(exact[k], model[k] if model is not None else None, exact["A"])
    return bound, e_q
