"""float64 reference of the inference pass of one PDRF level (VoxelNeRFBase.forward, networks/pdrf/voxnerf.py:210-259), the model of
the single-product half-precision modes, the bound every output of evd_voxel_forward is held to, and the case matrix of
tests/test_gpu_voxel_level_forward.py.  Test infrastructure only; nothing here needs a GPU (tests/test_voxel_level_ref.py).

level_forward64   the per-sample networks: raw [n, 4] = (sigma, sigmoid colours) and the geo rows [n, G], from the float32 values the
                  kernel gets.  quant=None is exact float64 and, at (10, 4), the arithmetic of torch_restatement.TorchVoxLevel.
                  quant="f16" / "bf16" is the MODEL of those modes: weights rounded to nearest in the type, the input of every linear
                  layer (features, both encodings, hidden activations after ReLU, the geo rows entering color_net.0) rounded to nearest in
                  the type (the kernels convert with the default rounding mode, mlp_pipe.h POps::set_pair), products and sums exact,
                  biases float32 values added in float64; sigma, the geo rows that are OUTPUT and the sigmoid are left unrounded.
level_outputs64   colour, depth, acc, weights and the feature output through composite_ref.composite (sigma channel 0, colours 1..3, the
                  level's activations, rmnear = render_rmnearplane / 128 outside training).  composite_feature levels in the reference's
                  order (voxnerf.py:223-239): activate the geo rows, composite them to [R, G], run the colour network per ray in float64
                  on cat([map, PE(dirs)]).  That network is float32 in every mode (k_color_rows), so `quant` never reaches it.
bounds            bound(X) = 4 E_q(X) + floor(X) + composite_ref's own E_X 2^-24, from the two float64 evaluations alone:
                  E_q(X)   L-inf distance of the quantised model's X from the exact one (0 in the float32-grade modes f32, f16x3, f16c);
                           4 = 2 (a kernel that truncates where the model rounds to nearest) x 2 (float32 accumulation, and a finite
                           sample under-reading the worst case);
                  F        5e-5 max(1, A): the project's float32-grade figure for these networks on raw against float64
                           (tests/test_gpu_train_f16c.py), A the largest absolute pre-activation of the float64 network in the case;
                  floor    F for per-sample outputs (feature rows; the weights of the unit-spacing layouts, where
                           w_i = T_i (1 - exp(-relu(sigma_i))) has a derivative of at most 1 in every sigma); F (1 + 2 D) max(1, V) for
                           composited ones: D the largest sum_j dist_j over the rays (sum_i |d w_i / d sigma_j| <= 2 dist_j), V the largest
                           magnitude being averaged (1 for colour and acc, max |z| for depth, max |activated geo| for the map).  With S = 1
                           D is 0 and the colour IS the sample's colour, so its floor is F.  The per-ray colour of a composite_feature
                           level is a network output behind the composited map; it takes the floor of the map (V = max |geo|): the three
                           layers' gain on this project's weights is below 1 (the geo faults of FAULTS move colours by less than they
                           move the rows).
Nothing measured on a kernel enters a bound.

CASES is the arm matrix: every case names the arm of voxel_level_forward (csrc/evd_voxel_render_api.hip) it reaches, and expected_arm()
re-derives that arm from the case's construction alone, mirroring the dispatch.

Layouts.  Per-sample (S <= 3): z = 0, 1, 2 on unit rays_d, one view direction per ray.  Per-ray: sorted uniform z in (0, 1) on N(0, 1)
ray directions.  Input condition of the per-sample cases (asserted on the reference in tests/test_voxel_level_ref.py): at least 25 % of
the samples have sigma > 0 and at least 25 % sigma <= 0 -- SEEDS records the weight seeds chosen for that on the CPU (seed 71 gives 19 %
on the fine level); the single sample of a 1 x 1 case cannot meet it and is exempt.  No reference pre-activation decides anything."""
import functools

import numpy as np
import torch

from composite_ref import ACT, _act, composite
from evdeblurnerf_amd import weights as W
from torch_restatement import embed

AABB = W.BLURFACTORY_AABB
QUANT = {"f16": torch.float16, "bf16": torch.bfloat16}
DIMS = {"coarse": dict(HD=64, G=15, FT=32, nvox=24 ** 3), "fine": dict(HD=256, G=128, FT=64, nvox=48 ** 3)}
U = 2.0 ** -24
F32_GRADE = 5e-5
RESIDENT_FROM = 65536               # samples from which the 64-wide level runs k_voxel_mlp_resident

# structural faults of the float64 restatement (what a packing or column-map mistake produces); tests/test_voxel_level_ref.py holds
# every bf16 bound of the per-sample cases below the change each of them makes
FAULTS = ("top_pts_freq", "top_pts_cos", "top_dir_freq", "last_ft", "last_hid", "first_geo", "last_geo", "geo_shift",
          "nobias_color_net.0", "nobias_color_net.1", "nobias_color_net.2")


def _t64(a, dev):
    return torch.as_tensor(a).to(device=dev, dtype=torch.float64)


def _dev(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor):
            return t.device
    return torch.device("cpu")


def level_forward64(sd, pts, dirs, fts, multires, multires_views, quant=None, fault=None, stats=None):
    """-> raw [n, 4], geo [n, G] (float64).  pts, dirs [n, 3], fts [n, FT]: numpy or torch, float32 values.  Absent color_net.*.bias keys
    mean no bias (the shipped configuration).  stats: a dict that receives "A", the largest absolute pre-activation."""
    dev = _dev(pts, dirs, fts)
    dt = QUANT[quant] if quant is not None else None
    q = (lambda x: x.to(dt).double()) if dt is not None else (lambda x: x)
    P = {k: _t64(np.asarray(v), dev) for k, v in sd.items() if k.startswith(("sigma_net.", "color_net."))}
    pre = []

    def lin(name, x):
        y = q(x) @ q(P[name + ".weight"]).T
        if name + ".bias" in P and fault != "nobias_" + name:
            y = y + P[name + ".bias"]
        pre.append(y)
        return y

    pts, dirs, fts = _t64(pts, dev).reshape(-1, 3), _t64(dirs, dev).reshape(-1, 3), _t64(fts, dev)
    fts = fts.reshape(pts.shape[0], -1)
    ep, ed = embed(pts, multires), embed(dirs, multires_views)
    if fault == "top_pts_freq":
        ep = ep.clone(); ep[:, -6:] = 0
    if fault == "top_pts_cos":
        ep = ep.clone(); ep[:, -3:] = 0
    if fault == "top_dir_freq":
        ed = ed.clone(); ed[:, -6:] = 0
    if fault == "last_ft":
        fts = fts.clone(); fts[:, -1] = 0
    h = torch.relu(lin("sigma_net.0", torch.cat([fts, ep], -1)))
    if fault == "last_hid":
        h = h.clone(); h[:, -1] = 0
    sg = lin("sigma_net.1", h)
    geo = sg[:, 1:]
    gin = geo
    if fault == "first_geo":
        gin = geo.clone(); gin[:, 0] = 0
    if fault == "last_geo":
        gin = geo.clone(); gin[:, -1] = 0
    if fault == "geo_shift":
        gin = torch.roll(geo, 1, 1)
    c = torch.relu(lin("color_net.0", torch.cat([gin, ed], -1)))
    c = torch.relu(lin("color_net.1", c))
    raw = torch.cat([sg[:, :1], torch.sigmoid(lin("color_net.2", c))], -1)
    if stats is not None:
        stats["A"] = max(float(y.abs().max()) for y in pre)
    return raw, geo


def color_rows64(sd, fmap, dirs, multires_views, stats=None):
    """the colour network of a composite_feature level per ray (voxnerf.py:231-239): ReLU, ReLU, sigmoid on cat([map, PE(dirs)])"""
    dev = fmap.device
    P = {k: _t64(np.asarray(v), dev) for k, v in sd.items() if k.startswith("color_net.")}
    h = torch.cat([fmap, embed(_t64(dirs, dev), multires_views)], -1)
    A = 0.0
    for l in range(3):
        h = h @ P[f"color_net.{l}.weight"].T
        if f"color_net.{l}.bias" in P:
            h = h + P[f"color_net.{l}.bias"]
        A = max(A, float(h.abs().max()))
        h = torch.relu(h) if l < 2 else torch.sigmoid(h)
    if stats is not None:
        stats["A"] = max(stats.get("A", 0.0), A)
    return h


def level_outputs64(raw, geo, z, rays_d, level_cfg, stats=None):
    """-> dict(color [R, 3], depth [R], acc [R], weights [R, S], feature [R, S, G] | [R, G], E = {name: composite_ref's bound, absolute}).
    level_cfg: rgb_activate, sigma_activate, render_rmnearplane, is_train, composite_feature and, for composite_feature levels, sd,
    viewdirs [R, 3] and multires_views of the per-ray colour network."""
    dev = raw.device
    z = _t64(z, dev)
    R, S = z.shape
    raw, geo = raw.reshape(R, S, 4), geo.reshape(R, S, -1)
    rm = float(level_cfg.get("render_rmnearplane", 0))
    rmnear = rm / 128.0 if (rm > 0 and not level_cfg.get("is_train", False)) else 0.0
    kw = dict(sigma_ch=0, rgb_ch0=1, n_rgb=3, rgb_act=level_cfg["rgb_activate"], sigma_act=level_cfg.get("sigma_activate", "relu"), rmnear=rmnear)
    if level_cfg.get("composite_feature", False):
        rows = _act(ACT[level_cfg["rgb_activate"]], geo, torch.zeros_like(geo))[0]
        c = composite(raw, z, rays_d, feature=rows, **kw)
        fmap = c["fmap"]
        color = color_rows64(level_cfg["sd"], fmap, level_cfg["viewdirs"], level_cfg["multires_views"], stats)
        feature, e_feat = fmap, float(c["E_fmap"].max()) * U
        e_col, vmap = e_feat, float(rows.abs().max())
    else:
        c = composite(raw, z, rays_d, **kw)
        color, feature, e_col, e_feat, vmap = c["rgb"], geo, float(c["E_rgb"].max()) * U, 0.0, 1.0
    return dict(color=color, depth=c["depth"], acc=c["acc"], weights=c["weights"], feature=feature, vmap=vmap,
                E=dict(color=e_col, depth=float(c["E_depth"].max()) * U, acc=float(c["E_acc"].max()) * U,
                       weights=float(c["E_weights"].max()) * U, feature=e_feat))


# ---- the case matrix ---------------------------------------------------------------------------------------------------------------
# weight seeds by (level, multires), chosen on the CPU: the first of 71, 72, .. whose share of sigma > 0 on the per-sample layouts lies
# in [0.25, 0.75] (coarse 0.29 / 0.40 / 0.52 at multires 10 / 7 / 0, fine 0.65 / 0.44 / 0.34)
SEEDS = {("coarse", 10): 71, ("coarse", 7): 71, ("coarse", 0): 73, ("fine", 10): 74, ("fine", 7): 71, ("fine", 0): 71}
OUTPUTS = ("color", "depth", "acc", "weights", "feature")


def case(arm, level, mode, R, S, entry, bias=True, ft_scale=0.3, enc=(10, 4), composite_feature=False, rgb_activate=None, rmnear=0,
         is_train=False, strides=False):
    """entry: "c" = the C entry with feature = NULL (as the c2f render calls a level), "forward" = VoxelNeRFBase.forward"""
    rgb_activate = rgb_activate or ("relu" if level == "coarse" else "none")
    cid = f"{arm}-{level}-{mode}-{R}x{S}" + ("" if bias else "-nobias") + ("" if ft_scale == 0.3 else f"-ft{ft_scale:g}")
    cid += ("" if enc == (10, 4) else f"-enc{enc[0]}_{enc[1]}") + (f"-{rgb_activate}" if composite_feature else "")
    cid += (f"-rmnear{rmnear}-train{int(is_train)}" if rmnear else "")
    return dict(id=cid, arm=arm, level=level, mode=mode, R=R, S=S, entry=entry, bias=bias, ft_scale=ft_scale, enc=tuple(enc),
                composite_feature=composite_feature, rgb_activate=rgb_activate, rmnear=rmnear, is_train=is_train, strides=strides)


def expected_arm(c):
    """the arm of voxel_level_forward a case reaches, from its construction (the dispatch of csrc/evd_voxel_render_api.hip restated)"""
    coarse, n = c["level"] == "coarse", c["R"] * c["S"]
    rows = c["composite_feature"] or (c["entry"] == "forward" and c["mode"] != "f16c")
    mode, rev = c["mode"], False
    if c["enc"] != (10, 4):
        return "generic_enc" if not c["composite_feature"] else "composite"       # no pipelined stream: f16c falls to f16x3's generic stream
    if mode == "f16c":
        if not coarse:
            return "pipe_c"
        mode, rev = "f16x3", True
    if mode != "f32" and not (coarse and rows):
        if not coarse:
            return "pipe_feat" if rows else "pipe"
        return ("resident_rev" if rev else "resident") if n >= RESIDENT_FROM else "pipe"
    return "composite" if c["composite_feature"] else "generic"


def _cases():
    out = []
    half, all4 = ("f16", "bf16", "f16x3"), ("f32", "f16x3", "f16", "bf16")
    for m in half:
        for (R, S), b in (((1, 1), False), ((2310, 1), True), ((1155, 2), False), ((70, 33), True), ((16512, 2), False)):
            out.append(case("pipe", "fine", m, R, S, "c", bias=b))
            out.append(case("pipe_feat", "fine", m, R, S, "forward", bias=b))
        for (R, S), b in (((1, 1), False), ((2310, 1), True), ((1155, 2), False), ((37, 131), True), ((4369, 15), False)):
            out.append(case("pipe", "coarse", m, R, S, "c", bias=b))
        for (R, S), b in (((1024, 64), True), ((1025, 64), False)):
            out.append(case("resident", "coarse", m, R, S, "c", bias=b))
    for (R, S), b in (((1, 1), False), ((2310, 1), True), ((770, 3), False), ((129, 127), True), ((16512, 2), False)):
        out.append(case("generic", "fine", "f32", R, S, "forward", bias=b))
    for (R, S), b in (((1, 1), False), ((16383, 1), True), ((770, 3), False), ((129, 127), True), ((16512, 2), False)):
        out.append(case("pipe_c", "fine", "f16c", R, S, "forward", bias=b))
    for (R, S), b in (((1024, 64), True), ((1025, 64), False)):
        out.append(case("resident_rev", "coarse", "f16c", R, S, "c", bias=b))
    for m in all4:
        for (R, S), b in (((1, 1), False), ((2310, 1), True), ((1155, 2), False), ((3, 43), True), ((16383, 1), False)):
            out.append(case("generic", "coarse", m, R, S, "forward", bias=b))
        for level in ("coarse", "fine"):
            for enc in ((7, 3), (0, 0)):
                for (R, S), b in (((1, 1), False), ((2310, 1), True), ((70, 33), False)):
                    out.append(case("generic_enc", level, m, R, S, "forward", bias=b, enc=enc))
        for act, enc in (("relu", (10, 4)), ("none", (10, 4)), ("relu", (10, 3))):
            for (R, S), b in (((1, 1), False), ((1155, 2), True), ((70, 33), True), ((37, 131), False)):
                out.append(case("composite", "coarse", m, R, S, "forward", bias=b, enc=enc, composite_feature=True, rgb_activate=act))
    for tr in (False, True):
        out.append(case("generic", "coarse", "f16x3", 70, 33, "forward", rmnear=32, is_train=tr))
        out.append(case("pipe", "coarse", "f16x3", 70, 33, "c", rmnear=32, is_train=tr))
    for m in ("f16x3", "f16"):
        for R, S in ((1, 1), (70, 33), (1155, 2)):
            out.append(case("pipe", "fine", m, R, S, "c", strides=True))
            out[-1]["id"] += "-strides"
    # features of scale 30: finiteness, and the bound with its magnitude term
    out.append(case("generic", "fine", "f32", 70, 33, "forward", ft_scale=30.0))
    out.append(case("pipe_feat", "fine", "f16x3", 70, 33, "forward", ft_scale=30.0))
    out.append(case("pipe_c", "fine", "f16c", 70, 33, "forward", ft_scale=30.0))
    out.append(case("generic", "coarse", "f32", 70, 33, "forward", ft_scale=30.0))
    out.append(case("generic", "coarse", "f16x3", 70, 33, "forward", ft_scale=30.0))
    out.append(case("pipe", "coarse", "f16c", 70, 33, "forward", ft_scale=30.0))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _state_dict(level, enc, bias):
    d = DIMS[level]
    gsz = W.pdrf_grid_size(AABB[0], AABB[1], d["nvox"])
    return W.make_pdrf_state_dict(SEEDS[(level, enc[0])], gsz, input_ch=d["FT"] + 3 * (1 + 2 * enc[0]), input_ch_views=3 * (1 + 2 * enc[1]),
                                  hidden_dim=d["HD"], geo_feat_dim=d["G"], add_bias_color=bias)


def state_dict(c):
    return _state_dict(c["level"], c["enc"], c["bias"])


@functools.lru_cache(maxsize=None)
def _inputs(level, R, S, ft_scale, rmnear):
    rs = np.random.RandomState(11 + R + 1000 * S)
    FT = DIMS[level]["FT"]
    pts = rs.uniform(-1, 1, (R, S, 3)).astype(np.float32)
    d = rs.normal(size=(R, 3))
    vd = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    fts = (ft_scale * rs.normal(size=(R, S, FT))).astype(np.float32)
    if S <= 3:
        z, rd = np.tile(np.arange(S, dtype=np.float32), (R, 1)), vd.copy()
    else:
        z, rd = np.sort(rs.uniform(0, 1, (R, S)).astype(np.float32), -1), rs.normal(size=(R, 3)).astype(np.float32)
    return dict(pts=pts, vd=vd, fts=fts, z=z, rd=rd)


def inputs(c):
    """float32 numpy inputs of a case: pts [R, S, 3], vd [R, 3] (unit), fts [R, S, FT], z [R, S], rd [R, 3]; shared, do not write"""
    return _inputs(c["level"], c["R"], c["S"], c["ft_scale"], c["rmnear"])


def evaluate(c, dev="cpu", quant=None, fault=None):
    """the float64 outputs of a case (level_outputs64 + raw, geo, A, D, max |z|, share of sigma > 0)"""
    sd, a = state_dict(c), inputs(c)
    R, S = c["R"], c["S"]
    t = {k: torch.as_tensor(v).to(dev) for k, v in a.items()}
    stats = {}
    with torch.no_grad():
        dirs = t["vd"][:, None].expand(R, S, 3).reshape(-1, 3)
        raw, geo = level_forward64(sd, t["pts"], dirs, t["fts"].reshape(R * S, -1), c["enc"][0], c["enc"][1], quant=quant, fault=fault, stats=stats)
        cfg = dict(rgb_activate=c["rgb_activate"], sigma_activate="relu", render_rmnearplane=c["rmnear"], is_train=c["is_train"],
                   composite_feature=c["composite_feature"], sd=sd, viewdirs=t["vd"], multires_views=c["enc"][1])
        out = level_outputs64(raw, geo, t["z"], t["rd"], cfg, stats)
    z64, n64 = t["z"].double(), t["rd"].double().norm(dim=-1)
    out.update(raw=raw, geo=geo, A=stats["A"], D=float(((z64[:, -1] - z64[:, 0]) * n64).max()), zmax=float(z64.abs().max()),
               share=float((raw[:, 0] > 0).double().mean()))
    return out


def bounds(c, dev="cpu", exact=None):
    """-> (exact outputs, {output name: bound}, {output name: E_q}).  Only the two float64 evaluations enter."""
    ex = exact if exact is not None else evaluate(c, dev)
    qm = evaluate(c, dev, quant=c["mode"]) if c["mode"] in QUANT else None
    F = F32_GRADE * max(1.0, ex["A"])
    per_sample_layout = c["S"] <= 3
    V = dict(color=ex["vmap"] if c["composite_feature"] else 1.0, acc=1.0, weights=1.0, depth=ex["zmax"], feature=ex["vmap"])
    bound, e_q = {}, {}
    for k in OUTPUTS:
        e_q[k] = float((qm[k] - ex[k]).abs().max()) if qm is not None else 0.0
        if (k == "feature" and not c["composite_feature"]) or (k == "weights" and per_sample_layout):
            floor = F
        else:
            floor = F * (1 + 2 * ex["D"]) * max(1.0, V[k])
        bound[k] = 4 * e_q[k] + floor + ex["E"][k]
    return ex, bound, e_q
