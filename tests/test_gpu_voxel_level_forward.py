"""Every arm of the PDRF level inference pass (evd_voxel_forward -> voxel_level_forward, csrc/evd_voxel_render_api.hip) against the float64
reference of tests/voxel_level_ref.py, at the sizes where its tiling, its column maps and its kernel thresholds change.

Arms (the first field of a case id; voxel_level_ref.expected_arm re-derives it from the case's construction, and run() asserts what the
construction implies -- which entry, whether feature rows exist, which side of the 65536-sample threshold):
  pipe          k_voxel_mlp_pipe without feature rows: the C entry with feature = NULL, fine level (f16 / bf16 / f16x3; also with viewdirs and
                rays_d as columns of an 11-column ray batch, "-strides") and coarse level below 65536 samples (4369 x 15 = 65535)
  pipe_feat     its FEAT instantiation: VoxelNeRFBase.forward on the fine level, rows [R, S, 128] compared
  pipe_c        the compensated kernel: forward(precision="f16c") on the fine level, feature output None
  resident      k_voxel_mlp_resident: coarse level, C entry, 1024 x 64 = 65536 and the ragged 1025 x 64
  resident_rev  its rev_trig instantiation: the same in f16c
  generic       k_voxel_mlp on its own stream: fine f32, and the coarse level whenever rows [R, S, 15] are wanted (forward(), all four modes)
  generic_enc   the same for multires / multires_views (7, 3) and (0, 0), both levels
  composite     composite_feature (PBE) coarse level: generic kernel, k_act_inplace (taken with rgb_activate="relu", skipped with "none"),
                the feature-compositing scan, k_color_rows (also with multires_views = 3); map [R, 15] and per-ray colour compared
Bounds: voxel_level_ref.bounds, fixed from the two float64 evaluations before the kernel runs (4 x the model error of the mode + the
float32-grade floor + the scan's own bound); what keeps them honest is tests/test_voxel_level_ref.py (every structural fault of the
restatement exceeds the bf16 bound).  The float64 reference runs in torch on the device.

Measured on one MI355X: the worst share (error / bound) of each arm over its cases and outputs, with the output it occurred on.
The half-precision arms sit at a share of ~0.25: their error IS the model's (bound = 4 x model + floor); the float32-grade arms use less
than 1 % of the floor, the compensated kernel 18 %.  (The module prints this table again at the end of every run.)
  arm           level   mode    cases  worst share  output    error      bound
  composite     coarse  bf16       12        0.247  feature   9.61e-04   3.90e-03
  composite     coarse  f16        12        0.228  weights   2.02e-04   8.84e-04
  composite     coarse  f16x3      12        0.001  color     4.81e-08   5.01e-05
  composite     coarse  f32        12        0.001  weights   8.72e-08   7.65e-05
  generic       coarse  bf16        5        0.248  feature   2.59e-03   1.05e-02
  generic       coarse  f16         5        0.234  feature   2.90e-04   1.24e-03
  generic       coarse  f16x3       8        0.002  feature   3.54e-06   2.26e-03
  generic       coarse  f32         6        0.003  feature   7.56e-06   2.26e-03
  generic       fine    f32         6        0.005  feature   3.92e-07   8.64e-05
  generic_enc   coarse  bf16        6        0.248  feature   2.14e-03   8.63e-03
  generic_enc   coarse  f16         6        0.235  feature   2.91e-04   1.24e-03
  generic_enc   coarse  f16x3       6        0.002  feature   1.15e-07   7.65e-05
  generic_enc   coarse  f32         6        0.002  feature   1.59e-07   7.35e-05
  generic_enc   fine    bf16        6        0.248  feature   1.77e-03   7.13e-03
  generic_enc   fine    f16         6        0.234  feature   2.38e-04   1.02e-03
  generic_enc   fine    f16x3       6        0.003  feature   1.74e-07   6.60e-05
  generic_enc   fine    f32         6        0.005  feature   3.47e-07   6.60e-05
  pipe          coarse  bf16        5        0.230  color     2.29e-04   9.98e-04
  pipe          coarse  f16         5        0.202  weights   1.79e-04   8.84e-04
  pipe          coarse  f16c        1        0.000  weights   1.81e-07   1.71e-02
  pipe          coarse  f16x3       7        0.001  color     4.81e-08   5.04e-05
  pipe          fine    bf16        5        0.247  weights   1.41e-03   5.73e-03
  pipe          fine    f16         8        0.222  weights   1.70e-04   7.66e-04
  pipe          fine    f16x3       8        0.001  weights   1.11e-07   8.69e-05
  pipe_c        fine    f16c        6        0.175  weights   1.36e-05   7.77e-05
  pipe_feat     fine    bf16        5        0.248  feature   2.06e-03   8.32e-03
  pipe_feat     fine    f16         5        0.241  feature   2.85e-04   1.19e-03
  pipe_feat     fine    f16x3       6        0.002  feature   1.66e-07   7.04e-05
  resident      coarse  bf16        2        0.161  weights   4.24e-04   2.63e-03
  resident      coarse  f16         2        0.043  weights   4.77e-05   1.11e-03
  resident      coarse  f16x3       2        0.000  weights   4.20e-07   8.77e-04
  resident_rev  coarse  f16c        2        0.000  weights   4.20e-07   8.77e-04
"""
import ctypes as C

import numpy as np
import pytest
import torch

import voxel_level_ref as V

pytestmark = pytest.mark.gpu

_NETS, _EXACT, RECORD = {}, {}, {}


def level(c, rmnear=None):
    """the level of a case, built like _level() of tests/test_gpu_train_f16c.py (coarse 64 / 15 / 32 on 24^3 voxels, fine 256 / 128 / 64 on 48^3)"""
    from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures, VoxelNeRFSampleFeatures
    rmnear = c["rmnear"] if rmnear is None else rmnear
    key = (c["level"], c["enc"], c["bias"], c["composite_feature"], c["rgb_activate"], rmnear)
    if key not in _NETS:
        d = V.DIMS[c["level"]]
        cls = VoxelNeRFRayFeatures if c["level"] == "coarse" else VoxelNeRFSampleFeatures
        _NETS[key] = cls(V.state_dict(c), "", V.AABB, num_layers=2, hidden_dim=d["HD"], geo_feat_dim=d["G"], num_layers_color=3,
                         input_ch=d["FT"] + 3 * (1 + 2 * c["enc"][0]), multires=c["enc"][0], multires_views=c["enc"][1], app_dim=32,
                         app_n_comp=(64, 16, 16), n_voxels=d["nvox"], rgb_activate=c["rgb_activate"], render_rmnearplane=rmnear,
                         composite_feature=c["composite_feature"], precision="f16x3")
    return _NETS[key]


def run(c, net=None, mode=None):
    """-> dict(color, depth, acc, weights, feature | None) of the kernel, through the entry the case names"""
    import evdeblurnerf_amd._lib as L
    net, mode = net or level(c), mode or c["mode"]
    R, S = c["R"], c["S"]
    a = {k: torch.tensor(v, device="cuda") for k, v in V.inputs(c).items()}
    if c["entry"] == "forward":
        out = net.forward(a["pts"], a["vd"], a["fts"], a["z"], a["rd"], is_train=c["is_train"], precision=mode)
        feat = out[4]
        if mode == "f16c":
            assert feat is None
        else:
            assert feat.shape == ((R, net.geo_feat_dim) if c["composite_feature"] else (R, S, net.geo_feat_dim))
    else:
        f32 = dict(dtype=torch.float32, device="cuda")
        nan = lambda *sh: torch.full(sh, float("nan"), **f32)
        color, depth, acc, wts, feat = nan(R, 3), nan(R), nan(R), nan(R, S), None
        need = int(L.lib().evd_voxel_forward_workspace_bytes(net._h, R, S))
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
        if c["strides"]:          # viewdirs and rays_d read in place from the [R, 11] ray batch, as the render calls a level
            rb = torch.zeros((R, 11), **f32)
            rb[:, 3:6], rb[:, 8:11] = a["rd"], a["vd"]
            vd_p, rd_p, stride = C.c_void_p(rb.data_ptr() + 8 * 4), C.c_void_p(rb.data_ptr() + 3 * 4), 11
        else:
            vd_p, rd_p, stride = L.ptr(a["vd"]), L.ptr(a["rd"]), 3
        L.check(L.lib().evd_voxel_forward(net._h, L.PREC[mode], L.ptr(a["pts"]), vd_p, stride, L.ptr(a["fts"]), a["fts"].shape[-1], L.ptr(a["z"]),
                                          rd_p, stride, R, S, int(c["is_train"]), L.ptr(color), L.ptr(depth), L.ptr(acc), L.ptr(wts), None,
                                          L.ptr(ws), need, L.stream_ptr()), "evd_voxel_forward")
        out = (color, depth, acc, wts, None)
    torch.cuda.synchronize()
    return dict(zip(V.OUTPUTS, out))


def exact(c):
    key = (c["level"], c["R"], c["S"], c["enc"], c["bias"], c["ft_scale"], c["composite_feature"], c["rgb_activate"], c["rmnear"], c["is_train"])
    if key not in _EXACT:
        _EXACT[key] = V.evaluate(c, "cuda")
    return _EXACT[key]


@pytest.fixture(scope="module", autouse=True)
def table():
    yield
    print("\n  arm           level   mode    cases  worst share  output    error      bound")
    for (arm, lv, mode), (n, share, k, err, b) in sorted(RECORD.items()):
        print(f"  {arm:13s} {lv:7s} {mode:6s} {n:6d}  {share:11.3f}  {k:8s}  {err:.2e}   {b:.2e}")
    _NETS.clear()
    _EXACT.clear()


@pytest.mark.parametrize("c", V.CASES, ids=[c["id"] for c in V.CASES])
def test_level_forward_arm_vs_float64(c):
    """every output of the arm within its bound of the float64 reference; the bound exists before the kernel runs"""
    n = c["R"] * c["S"]
    assert V.expected_arm(c) == c["arm"]
    if c["arm"].startswith("resident"):
        assert c["level"] == "coarse" and c["entry"] == "c" and n >= V.RESIDENT_FROM
    elif c["level"] == "coarse":
        assert n < V.RESIDENT_FROM
    ex, bound, e_q = V.bounds(c, "cuda", exact=exact(c))
    got = run(c)
    assert (got["feature"] is None) == (c["entry"] == "c" or c["mode"] == "f16c")
    errs = {}
    for k in V.OUTPUTS:
        if got[k] is None:
            continue
        assert got[k].shape == ex[k].shape and bool(torch.isfinite(got[k]).all()), k
        errs[k] = float((got[k].double() - ex[k]).abs().max())
        print(f"[{c['id']}] {k}: error {errs[k]:.3e}, bound {bound[k]:.3e} (model error {e_q[k]:.1e}), share {errs[k] / bound[k]:.3f}")
    k = max(errs, key=lambda k: errs[k] / bound[k])
    rec = RECORD.get((c["arm"], c["level"], c["mode"]), (0, -1.0, "", 0.0, 0.0))
    worst = (errs[k] / bound[k], k, errs[k], bound[k])
    RECORD[(c["arm"], c["level"], c["mode"])] = (rec[0] + 1,) + (worst if worst[0] > rec[1] else rec[1:])
    for k in errs:
        assert errs[k] <= bound[k], (c["id"], k, errs[k], bound[k])


def _same_bits(a, b, names=("color", "depth", "acc", "weights")):
    for k in names:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("level,enc,R,S,entry", [("coarse", (10, 4), 70, 33, "c"), ("coarse", (10, 4), 4369, 15, "c"),
                                                 ("coarse", (7, 3), 70, 33, "forward"), ("coarse", (0, 0), 2310, 1, "forward"),
                                                 ("fine", (7, 3), 70, 33, "forward"), ("fine", (0, 0), 2310, 1, "forward")])
def test_f16c_is_f16x3_where_no_compensated_kernel_exists(level, enc, R, S, entry):
    """the coarse level below 65536 samples (same entry: k_voxel_mlp_pipe has no rev_trig form), and either level under other encodings
    (the generic kernel, with and without rows): f16c gives the bits of f16x3.  (Through forward() at (10, 4) the two modes of the coarse
    level run DIFFERENT kernels -- f16x3 wants rows and takes the generic one -- and differ by an ulp of the colour: not compared.)"""
    c = V.case("x", level, "f16x3", R, S, entry, enc=enc)
    assert V.expected_arm(dict(c, mode="f16c")) in ("pipe", "generic_enc")
    _same_bits(run(c, mode="f16c"), run(c, mode="f16x3"))


@pytest.mark.parametrize("mode", ["f16", "bf16", "f16x3"])
@pytest.mark.parametrize("R,S", [(1, 1), (70, 33), (16512, 2)])
def test_fine_pipe_without_rows_is_the_feat_instantiation(mode, R, S):
    """colour, depth, acc and weights of k_voxel_mlp_pipe with and without its feature rows, bit for bit"""
    _same_bits(run(V.case("pipe", "fine", mode, R, S, "c")), run(V.case("pipe_feat", "fine", mode, R, S, "forward")))


@pytest.mark.parametrize("entry", ["c", "forward"])
def test_rmnear_masks_outside_training_only(entry):
    """render_rmnearplane = 32 with z in (0, 1): is_train = 0 masks the densities in front of 0.25, is_train = 1 equals a level built with
    render_rmnearplane = 0 bit for bit; the mask matters on these inputs (asserted on the reference)"""
    arm = "pipe" if entry == "c" else "generic"
    on, off = (V.case(arm, "coarse", "f16x3", 70, 33, entry, rmnear=32, is_train=t) for t in (False, True))
    ref_on, ref_off = V.evaluate(on, "cuda"), V.evaluate(off, "cuda")
    assert float((ref_on["weights"] - ref_off["weights"]).abs().max()) > 1e-2
    got_on, got_off = run(on), run(off)
    plain = run(off, net=level(off, rmnear=0))
    _same_bits(got_off, plain)
    assert float((got_on["weights"] - got_off["weights"]).abs().max()) > 1e-2
    front = torch.tensor(V.inputs(on)["z"][:, 1:] <= np.float32(0.25), device="cuda")
    assert bool((got_on["weights"][:, :-1][front] == 0).all())         # a masked density: alpha = 1 - exp(-0) = 0 exactly
