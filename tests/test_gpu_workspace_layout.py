"""Workspaces of the C ABI: every entry carves its workspace with ONE layout function that its *_workspace_bytes query shares
(csrc/evd_common.h Workspace).  Three properties per entry:
  sizes      the handle-bound queries equal a plain restatement of their slot lists (256-byte slots + the entry's slack)
  guard band the entry, given an UNALIGNED workspace pointer (base + 1, base + 255) and exactly the queried byte count, writes nothing from
             workspace + need on (a 0xA5 band of need + 512 - k bytes behind it stays intact) and computes what it computes on an aligned,
             larger workspace: bit for bit for the forward and once-per-dataset entries; for the pipelined backwards and the two scatter
             entries (float atomics, wavefront order) within the bound the entry's own test holds it to against its reference
  undersized need - 1 bytes -> EVD_E_WORKSPACE, the error text names the workspace, outputs and workspace untouched
The shapes are the smallest at which the layouts differ: 3 rays, 8 (+ 4) samples, 24 backward samples, 0 / 5 events on a 3 x 2 sensor, the
AWP tail (evd_awp_tail_forward / _backward) on 3 rays x 2 sub-exposures x 5 samples."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_awp as TA
import test_gpu_deterministic_scatter as TD
import test_gpu_train as TT
import test_gpu_triplane as T
from evdeblurnerf_amd import _lib as L, weights as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAT = 0xA5
E_WORKSPACE = -3
FILL = {torch.float32: 1234.5, torch.float64: 1234.5, torch.int64: 77, torch.int32: 77, torch.uint8: 0x5A}
R, S = 3, 8


def al(b):
    return (int(b) + 255) & ~255


def filled(shape, dtype=torch.float32):
    return torch.full(tuple(shape), FILL[dtype], dtype=dtype, device=DEV)


def untouched(t):
    return bool((t == FILL[t.dtype]).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def T_(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV).to(dtype) if dtype else torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def guard_band(need, run, compare=None, cleared=(), undersized=True):
    """run(ws_address, ws_bytes) -> (rc, {name: output}) on fresh pattern-filled outputs, synchronised.  cleared: outputs the entry resets
    before it looks at its workspace (flag words and per-pixel tables that every call starts from)."""
    need = int(need)
    assert need > 0
    big = torch.full((need + 4096,), PAT, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 256 == 0
    rc, ref = run(big.data_ptr(), need + 4096)
    assert rc == 0, L.lib().evd_last_error()
    for k in (1, 255):
        buf = torch.full((2 * need + 512,), PAT, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 512 == 0
        rc, out = run(buf.data_ptr() + k, need)
        assert rc == 0, L.lib().evd_last_error()
        assert bool((buf[k + need:] == PAT).all()), f"k = {k}: bytes written at or past workspace + need"
        assert bool((buf[:k] == PAT).all()), f"k = {k}: bytes written in front of the workspace"
        if compare is not None:
            compare(out, ref)
        else:
            for name in ref:
                assert same_bits(out[name], ref[name]), f"k = {k}: {name} differs from the aligned call"
    if undersized:
        buf = torch.full((need + 512,), PAT, dtype=torch.uint8, device=DEV)
        rc, out = run(buf.data_ptr() + 1, need - 1)
        assert rc == E_WORKSPACE
        msg = L.lib().evd_last_error()
        assert b"workspace" in msg and str(need - 1).encode() in msg and str(need).encode() in msg, msg
        for name, t in out.items():
            assert name in cleared or untouched(t), f"{name} written by a call that failed with EVD_E_WORKSPACE"
        assert bool((buf == PAT).all())


# ---- models ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nerf_model():
    from evdeblurnerf_amd.renderer import NeRFAll
    sd = dict(W.prefixed(W.make_nerf_state_dict(11), "mlp_coarse"))
    sd.update(W.prefixed(W.make_nerf_state_dict(12), "mlp_fine"))
    args = SimpleNamespace(mode="nerf", netdepth=8, netwidth=256, multires=10, multires_views=4, use_viewdirs=True, rgb_activate="sigmoid",
                           sigma_activate="relu", N_importance=4)
    return NeRFAll(args, sd, precision="f16x3").eval()


@functools.lru_cache(maxsize=None)
def pbe_model():
    """mode='c2f' with a composite_feature (kernel_type PBE) coarse level, as tests/test_gpu_parity.py builds it for golden G25"""
    from evdeblurnerf_amd.renderer import NeRFAll
    a = W.blurfactory_args(32, coarse_voxels=24 ** 3, fine_voxels=48 ** 3)
    a.kernel_type = "PBE"
    gc, gf = W.pdrf_grid_size(*W.BLURFACTORY_AABB, 24 ** 3), W.pdrf_grid_size(*W.BLURFACTORY_AABB, 48 ** 3)
    sd = W.prefixed(W.make_pdrf_state_dict(91, gc, input_ch=95, hidden_dim=64, geo_feat_dim=15), "mlp_coarse")
    sd.update(W.prefixed(W.make_pdrf_state_dict(92, gf, input_ch=127, hidden_dim=256, geo_feat_dim=128), "mlp_fine"))
    m = NeRFAll(a, sd, precision="f16x3").eval()
    assert m.mlp_coarse.composite_feature and not m.mlp_fine.composite_feature
    return m


@functools.lru_cache(maxsize=None)
def train_model():
    return TT._c2f_model("f16", 4)[0]


def render_cfg(model, Ni):
    return model._cfg(400, 400, float(W.synthetic_camera()[0][0]), True, 0., 1., S, Ni, False, 0., False)


def rays_and_batch(cfg):
    rays = T_(W.synthetic_rays(1, R), torch.float32).reshape(-1, 3, 2).contiguous()
    assert rays.shape[0] == R
    rb = torch.empty((R, 11), dtype=torch.float32, device=DEV)
    L.check(L.lib().evd_ray_batch(C.byref(cfg), L.ptr(rays), R, L.ptr(rb), L.stream_ptr()), "evd_ray_batch")
    return rays, rb


# ---- sizes of the handle-bound queries ----------------------------------------------------------------------------------------------
def composite_bytes(level, R_, S_):
    return al(R_ * S_ * level.geo_feat_dim * 4) + al(R_ * level.geo_feat_dim * 4) if level.composite_feature else 0


def c2f_bytes(coarse, fine, R_, S_, Ni):
    St, Nn = S_ + Ni, Ni if Ni else 1
    slots = [R_ * 11 * 4, R_ * S_ * 4, R_ * St * 4, R_ * St * 12, R_ * St * 64 * 4, R_ * S_ * 32 * 4, R_ * Nn * 32 * 4, R_ * Nn * 12, R_ * St * 4,
             R_ * St * 16, R_ * S_ * 4, R_ * St * 4, R_ * Nn * 4]
    b = sum(al(s) for s in slots) + composite_bytes(coarse, R_, S_)
    if fine is not None and Ni:
        b += composite_bytes(fine, R_, St)
    return b + 512


def grid_sizes(level):
    sz = (C.c_long * 7)()
    L.check(L.lib().evd_voxel_grid_sizes(level._h, sz), "evd_voxel_grid_sizes")
    return list(sz)


def hybrid_bytes(level, n):
    ctot = grid_sizes(level)[6] // level.app_dim           # basis_mat: app_dim x sum(n_comp)
    return al(n * ctot * 4) + al(n * 3 * 16) + 512         # rows_l | ltap (LTap: 16 bytes) | lmax word (256) + slack


def det_bytes(level, n, hybrid_ok=True):
    sz = grid_sizes(level)
    region = 256 + sum(al(e * 8) for e in sz[:6]) + al(512 * sz[6] * 4)        # max word | six 64-bit shadows | SD_BLOCKS x (app_dim x ctot) partials
    return max(region, hybrid_bytes(level, n) if hybrid_ok else 0) + 256


def test_handle_bound_size_queries_equal_their_slot_lists():
    lib, m, tm = L.lib(), pbe_model(), train_model()
    for model in (m, tm):
        c, f = model.mlp_coarse, model.mlp_fine
        for R_ in (0, 1, 3, 7, 1000):
            for S_, Ni in ((8, 0), (8, 4), (3, 4), (64, 64)):
                cfg = model._cfg(0, 0, 1.0, False, 0., 1., S_, Ni, False, 0., False)
                assert lib.evd_c2f_render_workspace_bytes(c._h, f._h, C.byref(cfg), R_) == c2f_bytes(c, f, R_, S_, Ni), (R_, S_, Ni)
                assert lib.evd_c2f_render_workspace_bytes(c._h, None, C.byref(cfg), R_) == c2f_bytes(c, None, R_, S_, Ni), (R_, S_, Ni)
            for level in (c, f):
                for S_ in (1, 8, 12):
                    assert lib.evd_voxel_forward_workspace_bytes(level._h, R_, S_) == al(R_ * S_ * 16) + composite_bytes(level, R_, S_) + 512
        for level in (c, f):
            for n in (1, 24, 1000):
                assert lib.evd_voxel_sample_bwd_workspace_bytes(level._h, n) == hybrid_bytes(level, n), n
                assert lib.evd_voxel_sample_bwd_det_workspace_bytes(level._h, n) == det_bytes(level, n), n
            assert lib.evd_voxel_sample_bwd_workspace_bytes(level._h, 0) == 0 and lib.evd_voxel_sample_bwd_det_workspace_bytes(level._h, 0) == 0
    cfg = m._cfg(0, 0, 1.0, False, 0., 1., 8, 4, False, 0., False)
    assert lib.evd_c2f_render_workspace_bytes(None, None, C.byref(cfg), 3) == 0 and lib.evd_c2f_render_workspace_bytes(m.mlp_coarse._h, None, None, 3) == 0
    assert lib.evd_c2f_render_workspace_bytes(m.mlp_coarse._h, None, C.byref(cfg), -1) == 0
    assert lib.evd_voxel_forward_workspace_bytes(None, 3, 8) == 0 and lib.evd_voxel_forward_workspace_bytes(m.mlp_coarse._h, 3, 0) == 0
    lvl = T.make_level("c12", "fine", 0.1)[0]               # (48, 12, 12): no hybrid form, the deterministic entry sizes for its region alone
    assert lib.evd_voxel_sample_bwd_det_workspace_bytes(lvl._h, 24) == det_bytes(lvl, 24, hybrid_ok=False)


# ---- the two renders -----------------------------------------------------------------------------------------------------------------
def render_run(model, Ni, packed, c2f):
    """the entry on rays (packed=False: evd_*_render) or on the ray batch (evd_*_render_rays); every optional output requested"""
    lib = L.lib()
    cfg = render_cfg(model, Ni)
    rays, rb = rays_and_batch(cfg)
    coarse, fine = model.mlp_coarse.handle, (model.mlp_fine.handle if Ni else None)
    if c2f:
        fn, need = (lib.evd_c2f_render_rays if packed else lib.evd_c2f_render), lib.evd_c2f_render_workspace_bytes(coarse, fine, C.byref(cfg), R)
    else:
        fn, need = (lib.evd_nerf_render_rays if packed else lib.evd_nerf_render), lib.evd_nerf_render_workspace_bytes(C.byref(cfg), R)
    St = S + Ni

    def run(ws, nbytes):
        o = dict(rgb=filled((R, 3)), depth=filled((R,)), acc=filled((R,)), z_vals=filled((R, St)), weights=filled((R, St)))
        if Ni:
            o.update(rgb0=filled((R, 3)), depth0=filled((R,)), acc0=filled((R,)), z_std=filled((R,)), z_vals0=filled((R, S)), weights0=filled((R, S)))
        out = L.RenderOut()
        for name, t in o.items():
            setattr(out, name, L.ptr(t))
        out.feature_kind = 1
        rc = fn(coarse, fine, C.byref(cfg), L.ptr(rb if packed else rays), R, None, None, None, None, C.byref(out), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    return need, run


@pytest.mark.parametrize("Ni", [0, 4])
@pytest.mark.parametrize("packed", [False, True], ids=["evd_nerf_render", "evd_nerf_render_rays"])
def test_nerf_render(packed, Ni):
    guard_band(*render_run(nerf_model(), Ni, packed, c2f=False))


@pytest.mark.parametrize("Ni", [0, 4])
@pytest.mark.parametrize("packed", [False, True], ids=["evd_c2f_render", "evd_c2f_render_rays"])
def test_c2f_render_with_a_composite_feature_coarse_level(packed, Ni):
    guard_band(*render_run(pbe_model(), Ni, packed, c2f=True))


def level_inputs(aabb, seed=3):
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(aabb[0]), np.asarray(aabb[1])
    pts = T_(rs.uniform(lo * 0.9, hi * 0.9, (R, S, 3)).astype(np.float32))
    d = rs.normal(size=(R, 3))
    vd = T_((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))
    return pts, vd, rs


def test_voxel_forward_of_a_composite_feature_level():
    lib, level = L.lib(), pbe_model().mlp_coarse
    pts, vd, rs = level_inputs(W.BLURFACTORY_AABB)
    fts = T_((0.3 * rs.normal(size=(R, S, 32))).astype(np.float32))
    z = T_(np.sort(rs.uniform(0.2, 2.0, (R, S)).astype(np.float32), -1))
    G = level.geo_feat_dim

    def run(ws, nbytes):
        o = dict(color=filled((R, 3)), depth=filled((R,)), acc=filled((R,)), weights=filled((R, S)), feature=filled((R, G)))
        rc = lib.evd_voxel_forward(level._h, L.PREC["f16x3"], L.ptr(pts), L.ptr(vd), 3, L.ptr(fts), 32, L.ptr(z), L.ptr(vd), 3, R, S, 0, L.ptr(o["color"]),
                                   L.ptr(o["depth"]), L.ptr(o["acc"]), L.ptr(o["weights"]), L.ptr(o["feature"]), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    guard_band(lib.evd_voxel_forward_workspace_bytes(level._h, R, S), run)


# ---- the training backwards ------------------------------------------------------------------------------------------------------------
def rel_l2_all(out, ref, tol, what):
    """every output within `tol` relative L2 of the aligned call's: the bound `what` holds the entry to against float64 autograd"""
    for name in ref:
        e = TT.rel_l2(out[name].double(), ref[name].double())
        assert e < tol, f"{name}: relative L2 {e:.2e} from the aligned call (bound {tol:g}, {what})"


def nerf_backward_case(net, prec):
    lib = L.lib()
    rb, z = TT.make_inputs(R, S, 6)
    rb, z = T_(rb), T_(z)
    d_raw = T_((np.random.RandomState(9).normal(size=(R, S, 4)) * 1e-3).astype(np.float32))
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).reshape(-1, 3).contiguous()
    blocks = net.param_blocks()
    need = lib.evd_nerf_backward_workspace_bytes_net(net._h, L.PREC[prec])

    def run(ws, nbytes):
        raw, store = net.mlpforward_train(rb, z, precision=prec)
        o = dict(flat=filled((net._nparam,)), d_pts=filled((R * S, 3)), d_dirs=filled((R * S, 3)))
        gs, base = L.NerfGrads(), o["flat"].data_ptr()
        gs.accumulate = 0
        for key, shape, off in blocks:
            name, kind = key.rsplit(".", 1)
            field = "_w" if kind == "weight" else "_b"
            if name.startswith("pts_linears."):
                getattr(gs, "pts" + field)[int(name.split(".")[1])] = base + 4 * off
            else:
                setattr(gs, {"views_linears.0": "views", "feature_linear": "feature", "alpha_linear": "alpha", "rgb_linear": "rgb"}[name] + field, base + 4 * off)
        rc = lib.evd_nerf_mlp_backward(net._h, L.PREC[prec], L.ptr(d_raw), R, S, L.ptr(store), store.numel(), C.byref(gs), L.ptr(pts),
                                       C.c_void_p(rb[:, 8:11].data_ptr()), 11, L.ptr(o["d_pts"]), L.ptr(o["d_dirs"]), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        flat = o.pop("flat")
        o.update({key: flat[off:off + int(np.prod(shape))] for key, shape, off in blocks})         # one entry per parameter tensor
        return rc, o
    return need, run


def test_nerf_mlp_backward_pipelined():
    from evdeblurnerf_amd.nerf import NeRF
    net = NeRF(W.make_nerf_state_dict(22), precision="f16")
    # tests/test_gpu_train.py test_mlp_backward_matches_torch_autograd: relative L2 < 4e-3 per tensor in f16
    guard_band(*nerf_backward_case(net, "f16"), compare=lambda o, r: rel_l2_all(o, r, 4e-3, "test_gpu_train.py::test_mlp_backward_matches_torch_autograd"))


def test_nerf_mlp_backward_generic():
    from evdeblurnerf_amd.nerf import NeRF
    net = NeRF(W.make_nerf_state_dict(31, 4, 64), D=4, W=64, precision="f16x3")
    need, run = nerf_backward_case(net, "f16x3")
    assert need == (8 << 20) * 4 + 512            # the generic backward's partials (nerf_train_generic.h GEN_WS_FLOATS)
    guard_band(need, run)                         # bit for bit


def test_voxel_mlp_backward():
    lib, level = L.lib(), train_model().mlp_fine
    pts, vd, rs = level_inputs(TT.AABB, 11)
    FT = level.ft_dim
    fts = T_((0.3 * rs.normal(size=(R, S, FT))).astype(np.float32))
    d_raw = T_((rs.normal(size=(R, S, 4)) * 1e-3).astype(np.float32))
    blocks = level.param_blocks()
    assert level.has_color_bias

    def run(ws, nbytes):
        raw, store = TT._level_train_forward(level, "f16", pts, vd, fts)
        o = dict(flat=filled((level._nparam,)), d_fts=filled((R * S, FT)), d_pts=filled((R * S, 3)), d_dirs=filled((R * S, 3)))
        gs, base = L.VoxelGrads(), o["flat"].data_ptr()
        gs.accumulate = 0
        for key, shape, off in blocks:
            name, idx, kind = key.split(".")
            getattr(gs, ("sigma_" if name == "sigma_net" else "color_") + ("w" if kind == "weight" else "b"))[int(idx)] = base + 4 * off
        rc = lib.evd_voxel_mlp_backward(level._h, L.PREC["f16"], L.ptr(d_raw), L.ptr(raw), None, None, 0, R, S, L.ptr(store), store.numel(), C.byref(gs),
                                        L.ptr(o["d_fts"]), FT, L.ptr(pts), L.ptr(vd), 3, L.ptr(o["d_pts"]), L.ptr(o["d_dirs"]), C.c_void_p(ws), nbytes,
                                        L.stream_ptr())
        torch.cuda.synchronize()
        flat = o.pop("flat")
        o.update({key: flat[off:off + int(np.prod(shape))] for key, shape, off in blocks})         # one entry per parameter tensor
        return rc, o
    # tests/test_gpu_train.py test_pdrf_level_networks_backward_match_torch_autograd: relative L2 < 4e-3 per tensor in f16
    guard_band(lib.evd_voxel_backward_workspace_bytes(), run,
               compare=lambda o, r: rel_l2_all(o, r, 4e-3, "test_gpu_train.py::test_pdrf_level_networks_backward_match_torch_autograd"))


def test_awp_embed_backward():
    lib = L.lib()
    emb, flat, ws_, bs_ = TA._embed("f16")
    n = R * S
    rs = np.random.RandomState(7)
    x = T_((rs.standard_normal((n, 128)) * 0.7).astype(np.float32))
    g = T_((rs.standard_normal((n, 64)) * 1e-4).astype(np.float32))
    nb = int(lib.evd_awp_embed_store_bytes(emb._h, n))

    def run(ws, nbytes):
        store = torch.zeros((nb,), dtype=torch.uint8, device=DEV)
        h = torch.empty((n, 64), dtype=torch.float32, device=DEV)
        L.check(lib.evd_awp_embed_forward(emb._h, L.PREC["f16"], L.ptr(x), None, None, 0, n, L.ptr(h), L.ptr(store), nb, L.stream_ptr()), "evd_awp_embed_forward")
        o = dict(flat=filled((emb.nparam,)), d_rows=filled((n, 128)))
        gs, base = L.AwpEmbedGrads(), o["flat"].data_ptr()
        for l, (wo, bo) in enumerate(emb.offsets):
            gs.w[l], gs.b[l] = base + 4 * wo, base + 4 * bo
        rc = lib.evd_awp_embed_backward(emb._h, L.PREC["f16"], L.ptr(g), n, L.ptr(store), nb, C.byref(gs), L.ptr(o["d_rows"]), None, C.c_void_p(ws), nbytes,
                                        L.stream_ptr())
        torch.cuda.synchronize()
        flat = o.pop("flat")
        for l, (wo, bo) in enumerate(emb.offsets):              # one entry per parameter tensor
            o[f"w{l}"], o[f"b{l}"] = flat[wo:bo], flat[bo:bo + 64]
        return rc, o
    # tests/test_gpu_awp.py test_sample_embed_backward_matches_torch_autograd: relative L2 < 4e-3 per tensor in f16
    guard_band(lib.evd_awp_embed_backward_workspace_bytes(), run,
               compare=lambda o, r: rel_l2_all(o, r, 4e-3, "test_gpu_awp.py::test_sample_embed_backward_matches_torch_autograd"))


# ---- the AWP tail --------------------------------------------------------------------------------------------------------------------
TAIL_P, TAIL_S, TAIL_VF, TAIL_F, TAIL_NMOT = 2, 5, 3, 2, 2


def tail_case():
    """3 rays x 2 sub-exposures x 5 samples, view_feature 3 + 15 direction columns, two motion layers, training mode; the parameter
    tensors in the order include/evdnerf.h documents"""
    lib, P, S, VF = L.lib(), TAIL_P, TAIL_S, TAIL_VF
    desc = L.AwpTailDesc(P=P, S=S, VF=VF, dir_freqs=TAIL_F, n_mot=TAIL_NMOT, training=1, bn_eps=1e-5, bn_momentum=0.1)
    in0 = 64 + VF + 3 + 6 * TAIL_F
    sizes = [32 * in0, 32, 32 * 32, 32, 32 * 64, 32, 16 * 32, 16 * 32, 16 * 32, 16 * 16, 16 * 16, 32 * 32, 32, 32, P * 32, P]
    assert lib.evd_awp_tail_num_params(TAIL_NMOT) == len(sizes) and lib.evd_awp_tail_param_count(C.byref(desc)) == sum(sizes)
    rs = np.random.RandomState(21)
    params = [T_((0.2 * rs.standard_normal(n)).astype(np.float32)) for n in sizes]
    arr = (C.c_void_p * len(params))(*[t.data_ptr() for t in params])
    ins = dict(h=(R, P, 64), vf=(R, VF), rd=(R * P, 3), hi=(R, P, 64), hs=(R, S, 64), d_out=(R, P))
    ins = {k: T_(rs.standard_normal(sh).astype(np.float32)) for k, sh in ins.items()}
    return lib, desc, params, arr, ins, sum(sizes)


def tail_forward_run(lib, desc, arr, ins):
    nsaved = lib.evd_awp_tail_saved_floats(C.byref(desc))

    def run(ws, nbytes):
        o = dict(out=filled((R, TAIL_P)), y=filled((R, TAIL_P, 32)), xg=filled((R, TAIL_P, 32)), stats=filled((64,)), rays=filled((R, nsaved)),
                 run_mean=filled((32,)), run_var=filled((32,)), num_batches=filled((1,), torch.int64))
        rc = lib.evd_awp_tail_forward(C.byref(desc), arr, L.ptr(ins["h"]), L.ptr(ins["vf"]), L.ptr(ins["rd"]), L.ptr(ins["hi"]), L.ptr(ins["hs"]), R,
                                      L.ptr(o["run_mean"]), L.ptr(o["run_var"]), L.ptr(o["num_batches"]), L.ptr(o["out"]), L.ptr(o["y"]), L.ptr(o["xg"]),
                                      L.ptr(o["stats"]), L.ptr(o["rays"]), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    return run


def test_awp_tail_sizes_equal_their_slot_lists():
    lib, desc, params, arr, ins, total = tail_case()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for R_ in (0, 1, 3, 7, 1000):
        grid, nblk = min(max(R_, 1), cus), (R_ + 7) // 8           # a workgroup per ray up to one per CU; eight rays per finish workgroup
        assert lib.evd_awp_tail_workspace_bytes(C.byref(desc), R_, 0) == al(grid * 64 * 8) + 256, R_          # bn_part (double) + slack
        want = al(R_ * TAIL_P * 32 * 4) + al(nblk * (64 + TAIL_P * 32 + TAIL_P) * 4) + al(grid * ((total + 3) & ~3) * 4) + 256      # dz | partB | partA + slack
        assert lib.evd_awp_tail_workspace_bytes(C.byref(desc), R_, 1) == want, R_
    assert lib.evd_awp_tail_workspace_bytes(None, 3, 0) == 0 and lib.evd_awp_tail_workspace_bytes(C.byref(desc), -1, 1) == 0


def test_awp_tail_forward():
    lib, desc, params, arr, ins, total = tail_case()
    def compare(out, ref):
        # no atomics: bit for bit.  saved_rays is a copy of the ray's LDS block, padding included (row pads, 16-byte rounding of the arrays):
        # those floats are whatever the LDS held, so the block is checked by test_awp_tail_backward, which computes from it
        for name in ref:
            assert name == "rays" or same_bits(out[name], ref[name]), f"{name} differs from the aligned call"
    guard_band(lib.evd_awp_tail_workspace_bytes(C.byref(desc), R, 0), tail_forward_run(lib, desc, arr, ins), compare=compare)


def test_awp_tail_backward():
    lib, desc, params, arr, ins, total = tail_case()
    fwd_need = int(lib.evd_awp_tail_workspace_bytes(C.byref(desc), R, 0))
    fws = torch.empty((fwd_need,), dtype=torch.uint8, device=DEV)
    rc, f = tail_forward_run(lib, desc, arr, ins)(fws.data_ptr(), fwd_need)
    assert rc == 0, lib.evd_last_error()

    def run(ws, nbytes):
        o = dict(d_h=filled((R, TAIL_P, 64)), d_vf=filled((R, TAIL_VF)), d_rd=filled((R * TAIL_P, 3)), d_hi=filled((R, TAIL_P, 64)), d_hs=filled((R, TAIL_S, 64)),
                 d_params=filled((total,)))
        rc = lib.evd_awp_tail_backward(C.byref(desc), arr, L.ptr(ins["h"]), L.ptr(ins["vf"]), L.ptr(ins["rd"]), L.ptr(ins["hi"]), L.ptr(ins["hs"]), R, L.ptr(f["y"]),
                                       L.ptr(f["xg"]), L.ptr(f["stats"]), L.ptr(f["rays"]), L.ptr(ins["d_out"]), L.ptr(o["d_h"]), L.ptr(o["d_vf"]), L.ptr(o["d_rd"]),
                                       L.ptr(o["d_hi"]), L.ptr(o["d_hs"]), L.ptr(o["d_params"]), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    guard_band(lib.evd_awp_tail_workspace_bytes(C.byref(desc), R, 1), run)          # no atomics: bit for bit


# ---- the two scatter entries -------------------------------------------------------------------------------------------------------
def scatter_case(det):
    """the 'shipped' level, points and float64 reference of tests/test_gpu_deterministic_scatter.py (grid scale 0.1), f32 grids"""
    c = TD.case("shipped", "f32", 1)
    lvl, n = c["lvl"], c["pts"].shape[0]
    p, g = T_(c["pts"]), T_(c["d_out"])
    lib = L.lib()
    need = lib.evd_voxel_sample_bwd_det_workspace_bytes(lvl.handle, n) if det else lib.evd_voxel_sample_bwd_workspace_bytes(lvl.handle, n)

    def run(ws, nbytes):
        gp = [torch.zeros(pl.shape, dtype=torch.float32, device=DEV) for pl in c["planes"]]
        gl = [torch.zeros(li.shape, dtype=torch.float32, device=DEV) for li in c["lines"]]
        gb = torch.zeros(c["basis"].shape, dtype=torch.float32, device=DEV)
        dp = filled((n, 3))
        gs = L.VoxelGridGrads()
        for i in range(3):
            gs.plane[i], gs.line[i] = gp[i].data_ptr(), gl[i].data_ptr()
        gs.basis = gb.data_ptr()
        if det:
            rc = lib.evd_voxel_sample_bwd_det(lvl.handle, L.PREC["f32"], L.ptr(p), n, L.ptr(g), T.F, 0, C.byref(gs), L.ptr(dp), C.c_void_p(ws), nbytes, L.stream_ptr())
        else:
            rc = lib.evd_voxel_sample_bwd_ws(lvl.handle, L.ptr(p), n, L.ptr(g), T.F, 0, C.byref(gs), L.ptr(dp), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, dict(gp=gp, gl=gl, gb=gb, dp=dp)
    return c, n, need, run


def as_reference(c, aligned):
    """the float64 reference's magnitudes and counts with the aligned call's values in place of its sums"""
    r = dict(c["ref"])
    r["d_plane"], r["d_line"], r["d_basis"], r["d_pts"] = [t.double() for t in aligned["gp"]], [t.double() for t in aligned["gl"]], aligned["gb"].double(), aligned["dp"].double()
    return r


def scatter_untouched(o):
    assert all(float(t.abs().max()) == 0 for t in o["gp"] + o["gl"] + [o["gb"]]) and untouched(o["dp"])


def run_scatter(det):
    c, n, need, run = scatter_case(det)
    need = int(need)
    ct = sum(T.SHAPES["shipped"])
    kernel = T.bwd_kernel("shipped", "bwd_ws", False, True)

    def compare(out, ref):
        r = as_reference(c, ref)
        if det:         # tests/test_gpu_deterministic_scatter.py check_det: (KD + 4) u M + cnt unit, d basis 12 + n / 16 + 64, d pts KD + 3 ct + 16
            TD.check_det("unaligned vs aligned", r, c["unit"], out["gp"], out["gl"], out["gb"], out["dp"], n, ct)
        else:           # tests/test_gpu_triplane.py check_bwd: (kd + cnt + 2) u M planes, (kd + cnt + 4) u M + fixed point lines, d basis, d pts
            T.check_bwd("unaligned vs aligned", kernel, r, out["gp"], out["gl"], out["gb"], out["dp"], n, ct)
    big = torch.full((need + 4096,), PAT, dtype=torch.uint8, device=DEV)
    rc, ref = run(big.data_ptr(), need + 4096)
    assert rc == 0, L.lib().evd_last_error()
    assert float(ref["gp"][0].abs().max()) > 0
    for k in (1, 255):
        buf = torch.full((2 * need + 512,), PAT, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 512 == 0
        rc, out = run(buf.data_ptr() + k, need)
        assert rc == 0, L.lib().evd_last_error()
        assert bool((buf[k + need:] == PAT).all()) and bool((buf[:k] == PAT).all()), k
        compare(out, ref)
    buf = torch.full((need + 512,), PAT, dtype=torch.uint8, device=DEV)
    rc, out = run(buf.data_ptr() + 1, need - 1)
    assert rc == E_WORKSPACE and b"workspace" in L.lib().evd_last_error()
    scatter_untouched(out)
    assert bool((buf == PAT).all())


def test_voxel_sample_bwd_hybrid():
    run_scatter(det=False)


def test_voxel_sample_bwd_det():
    run_scatter(det=True)


# ---- the once-per-dataset entries ------------------------------------------------------------------------------------------------------
H_, W_ = 2, 3
HW = H_ * W_


def event_stream(N):
    rs = np.random.RandomState(5)
    x = rs.randint(0, W_, N).astype(np.float32) + (0.25 if N else 0)        # float coordinates: the colour map goes through its workspace
    y = rs.randint(0, H_, N).astype(np.float32) + (0.5 if N else 0)
    t = np.sort(rs.uniform(100, 400, N))
    p = rs.randint(0, 2, N).astype(np.float64)
    return T_(x), T_(y), T_(t), T_(p)


def coord_ids_run(N):
    lib = L.lib()
    x, y, _, _ = event_stream(N)

    def run(ws, nbytes):
        o = dict(ev_ids=filled((max(N, 1),), torch.int64), noev=filled((HW,), torch.int64), i2c=filled((N + HW, 2), torch.float64), counts=filled((2,), torch.int64))
        rc = lib.evd_event_coord_ids(L.ptr(x), L.ptr(y), N, H_, W_, L.ptr(o["ev_ids"]), L.ptr(o["noev"]), L.ptr(o["i2c"]), L.ptr(o["counts"]), C.c_void_p(ws),
                                     nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    return lib.evd_event_coord_ids_workspace_bytes(N, H_, W_), run


@pytest.mark.parametrize("N", [0, 5])
def test_event_coord_ids(N):
    guard_band(*coord_ids_run(N))


@pytest.mark.parametrize("N", [0, 5])
def test_event_filter(N):
    lib = L.lib()
    _, _, t, p = event_stream(N)
    ids = T_(np.arange(N, dtype=np.int64) % 3)

    def run(ws, nbytes):
        o = dict(ev3=filled((max(N, 1), 3), torch.float64), count=filled((1,), torch.int64), bad=filled((1,), torch.int32))
        rc = lib.evd_event_filter(L.ptr(ids), L.ptr(t), L.ptr(p), N, 150.0, 350.0, L.ptr(o["ev3"]), L.ptr(o["count"]), L.ptr(o["bad"]), C.c_void_p(ws), nbytes,
                                  L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    # N == 0 returns before the workspace is looked at; bad_polarity is reset on entry
    guard_band(lib.evd_event_filter_workspace_bytes(N), run, cleared=("bad",), undersized=N > 0)


@pytest.mark.parametrize("N", [0, 5])
def test_event_color_map(N):
    lib = L.lib()
    nb, coord_ids = coord_ids_run(N)
    ws0 = torch.empty((int(nb) + 256,), dtype=torch.uint8, device=DEV)
    rc, tab = coord_ids(ws0.data_ptr(), int(nb) + 256)          # the coordinate table of the stream: this entry's input
    assert rc == 0
    n_coords, n_noev = (int(v) for v in tab["counts"].tolist())
    i2c, noev = tab["i2c"][:n_coords].contiguous(), tab["noev"][:max(n_noev, 1)].contiguous()
    mx = T_((np.arange(HW).reshape(H_, W_) % W_).astype(np.float32) + 0.25)
    my = T_((np.arange(HW).reshape(H_, W_) // W_).astype(np.float32) + 0.5)
    assert n_coords > 0

    def run(ws, nbytes):
        o = dict(cmap=filled((n_coords, 3), torch.uint8), unmapped=filled((1,), torch.int32))
        rc = lib.evd_event_color_map(L.ptr(i2c), n_coords, H_, W_, L.ptr(mx), L.ptr(my), L.ptr(noev), n_noev, L.ptr(o["cmap"]), L.ptr(o["unmapped"]), C.c_void_p(ws),
                                     nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    guard_band(lib.evd_event_color_map_workspace_bytes(n_coords), run, cleared=("unmapped",))          # (unmapped is reset on entry)


@pytest.mark.parametrize("N", [0, 5])
def test_compute_successor(N):
    lib = L.lib()
    ids = T_(np.random.RandomState(3).randint(0, HW, max(N, 1)).astype(np.int32))

    def run(ws, nbytes):
        o = dict(succ=filled((max(N, 1),), torch.int64), nsucc=filled((max(N, 1),), torch.int32), latest=filled((HW,), torch.int64), first=filled((HW,), torch.int64))
        rc = lib.evd_compute_successor(L.ptr(ids), N, HW, L.ptr(o["succ"]), L.ptr(o["nsucc"]), L.ptr(o["latest"]), L.ptr(o["first"]), C.c_void_p(ws), nbytes,
                                       L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    # the two per-pixel tables are reset on entry; N == 0 returns before the workspace is looked at
    guard_band(lib.evd_compute_successor_workspace_bytes(N), run, cleared=("latest", "first"), undersized=N > 0)


def edi_run(n_img, chunk_images):
    lib = L.lib()
    steps, h, w, N = 3, 2, 3, 5
    rs = np.random.RandomState(8)
    ev = np.zeros((N, 4))
    ev[:, 0], ev[:, 1], ev[:, 2] = rs.randint(0, h * w, N), np.sort(rs.uniform(0, 1, N)), rs.choice([-1.0, 1.0], N)
    i2c = np.stack([np.arange(h * w) % w, np.arange(h * w) // w], 1).astype(np.float64)
    bounds = np.stack([np.linspace(0.1 * i, 0.1 * i + 0.6, steps) for i in range(n_img)])
    img = rs.uniform(0.1, 1.0, (n_img, h, w, 3)).astype(np.float32)
    ev, i2c, bounds, img = T_(ev), T_(i2c), T_(bounds), T_(img)

    def run(ws, nbytes):
        o = dict(prior=filled((n_img, h, w, 3)), windows=filled((2, n_img, steps), torch.int64), bad=filled((1,), torch.int32))
        rc = lib.evd_edi_prior(L.ptr(ev), N, L.ptr(i2c), h * w, L.ptr(bounds), L.ptr(img), n_img, steps, h, w, 0.2, 0.25, L.ptr(o["prior"]), L.ptr(o["windows"]),
                               L.ptr(o["bad"]), C.c_void_p(ws), nbytes, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, o
    return lib.evd_edi_prior_workspace_bytes(chunk_images, steps, h, w), run


@pytest.mark.parametrize("n_img,chunk_images", [(1, 1), (3, 1)], ids=["one_image", "three_images_in_chunks_of_one"])
def test_edi_prior(n_img, chunk_images):
    need, run = edi_run(n_img, chunk_images)
    guard_band(need, run, undersized=False)
    # A workspace below one image's is refused as a bad argument (EVD_E_INVALID, tests/test_edi_prior_cabi.py): the entry's code since it
    # was written, with the entry name, "workspace" and both byte counts in the text; nothing is written
    buf = torch.full((int(need) + 512,), PAT, dtype=torch.uint8, device=DEV)
    rc, out = run(buf.data_ptr() + 1, int(need) - 1)
    msg = L.lib().evd_last_error()
    assert rc == -1 and b"evd_edi_prior" in msg and b"workspace" in msg and str(int(need) - 1).encode() in msg and str(int(need)).encode() in msg
    assert all(untouched(t) for t in out.values()) and bool((buf == PAT).all())
    if n_img == 3:          # the chunked result is the one-pass result
        full_need, _ = edi_run(3, 3)
        big = torch.full((int(full_need) + 256,), PAT, dtype=torch.uint8, device=DEV)
        small = torch.full((int(need) + 256,), PAT, dtype=torch.uint8, device=DEV)
        a, b = run(big.data_ptr(), int(full_need))[1], run(small.data_ptr(), int(need))[1]
        assert all(same_bits(a[k], b[k]) for k in a)
