"""CPU-only: SparseBlurKernel carries the reference BlurModel's parameter names, shapes and initialisation (so a reference checkpoint's
kernelsnet.* keys load), and the three C entries validate their arguments before they touch a device."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
import sparse_blur_ref as SR

EXTRA = {"dsk": {}, "dsk_full": dict(spatial_embed=2, random_hwindow=0.0), "dsk_sv": {}, "pbe": dict(spatial_embed=2)}


@pytest.mark.parametrize("tag", SR.G39_CASES)
def test_reference_state_dict_loads_under_its_own_names(tag):
    from evdeblurnerf_amd.blurmodel import SparseBlurKernel
    c = SR.g39_case(load_golden("G39_sparse_blur"), tag)
    sd, cfg = c["params"], c["cfg"]
    for prefix in ("", "kernelsnet."):
        mod = SparseBlurKernel.from_state_dict({prefix + k: v for k, v in sd.items()}, cfg["kernel_type"], cfg["kernel_hwindow"], prefix=prefix, **EXTRA[tag])
        assert set(mod.state_dict()) == set(sd) == set(SR.param_keys(cfg, with_poses="poses" in sd))
        assert all(np.array_equal(v.numpy(), sd[k]) for k, v in mod.state_dict().items())
        assert {k for k, _ in mod.named_parameters()} == set(SR.param_keys(cfg))
        got = dict(num_pt=mod.num_pt, num_hidden=mod.num_hidden, num_wide=mod.num_wide, short_cut=int(mod.short_cut), isglobal=int(mod.isglobal),
                   optim_trans=int(mod.optim_trans), optim_spatialvariant_trans=int(mod.optim_sv_trans), in_embed=mod.in_embed, spatial_embed=mod.spatial_embed)
        assert got == {k: cfg[k] for k in got}
        assert (mod.poses is not None) == ("poses" in sd) and (cfg["kernel_type"] != "PBE" or mod.feat_cnl == 15)
    kw = {k: cfg[k] for k in ("random_hwindow", "in_embed", "spatial_embed", "num_hidden", "num_wide", "feat_cnl")}
    kw.update({k: bool(cfg[k]) for k in ("short_cut", "isglobal", "optim_trans", "optim_spatialvariant_trans")})
    strict = SparseBlurKernel(7, cfg["num_pt"], cfg["kernel_hwindow"], cfg["kernel_type"], poses=sd.get("poses"), **kw)
    strict.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)


def test_initialisation_and_from_args():
    """blurmodel.py:55-68,106-107 and utils/misc.py:95-102: pattern_pos ~ N(0, 1) pattern_init_radius, pattern_trans 0, Xavier-normal weights
    (gain 0.1 for the 3-row head, 1 elsewhere: std = gain sqrt(2 / (fan_in + fan_out))), biases 0; run_nerf.py:184-203: the flags' names"""
    from evdeblurnerf_amd.blurmodel import SparseBlurKernel
    args = SimpleNamespace(kernel_type="DSK", kernel_img_embed_type="param", kernel_img_embed=32, kernel_img_embed_init="zero", kernel_ptnum=5,
                           kernel_hwindow=10, kernel_random_hwindow=0.25, kernel_rand_embed=3, kernel_random_mode="input", kernel_spatial_embed=0,
                           kernel_depth_embed=0, kernel_num_hidden=3, kernel_num_wide=64, kernel_feat_cnl=15, kernel_shortcut=False,
                           kernel_pattern_init_radius=0.1, kernel_isglobal=False, kernel_global_trans=True, kernel_spatialvariant_trans=False)
    torch.manual_seed(5)
    mod = SparseBlurKernel.from_args(args, 34)
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    assert shapes == {"pattern_pos": (34, 5, 2), "pattern_trans": (34, 5, 2), "img_embed.img_embed": (34, 32), "linears.0.weight": (64, 46),
                      "linears.0.bias": (64,), "linears.2.weight": (64, 64), "linears.2.bias": (64,), "linears.4.weight": (64, 64), "linears.4.bias": (64,),
                      "linears1.0.weight": (64, 64), "linears1.0.bias": (64,), "linears1.2.weight": (3, 64), "linears1.2.bias": (3,)}
    assert 0.08 < mod.pattern_pos.std() < 0.12 and not mod.pattern_trans.any() and not mod.img_embed.img_embed.any()
    for name, gain, fan in (("linears.0", 1.0, 46 + 64), ("linears.2", 1.0, 128), ("linears1.0", 1.0, 128), ("linears1.2", 0.1, 67)):
        lin = mod.get_submodule(name)
        std = gain * (2.0 / fan) ** 0.5
        assert 0.8 * std < lin.weight.std() < 1.2 * std and not lin.bias.any(), name
    assert mod.kernel_hwindow == 10 and mod.random_hwindow == 0.25 and mod.kernel_type == "DSK" and mod.num_pt == 5
    sv = SparseBlurKernel(3, 4, 10, "PBE", optim_spatialvariant_trans=True, short_cut=True, spatial_embed=2, isglobal=True)
    assert sv.linears1[2].weight.shape == (5, 64) and sv.linears1[0].weight.shape == (64, 64 + 14 + 32 + 15 + 10) and sv.pattern_pos.shape == (1, 4, 2)
    assert sv.linears1[2].weight.std() > 0.1                                          # 5 rows: the full gain


def test_what_is_not_built_is_refused_in_python():
    from evdeblurnerf_amd._lib import EvdError
    from evdeblurnerf_amd.blurmodel import SparseBlurKernel
    with pytest.raises(EvdError, match="depth_embed"):
        SparseBlurKernel(3, 5, 10, "DSK", depth_embed=2)
    with pytest.raises(EvdError, match="use_pattern_pos"):
        SparseBlurKernel(3, 5, 10, "DSK", use_pattern_pos=False)
    with pytest.raises(EvdError, match="kernel_type"):
        SparseBlurKernel(3, 5, 10, "RBK")
    mod = SparseBlurKernel(3, 5, 10, "DSK", random_mode="output")
    with pytest.raises(NotImplementedError, match="output"):
        mod(4, 4, np.eye(3), None, {"images_idx": torch.zeros((2, 1), dtype=torch.int64)})


OK = dict(kernel_type=0, num_pt=5, in_embed=3, spatial_embed=0, embed_cnl=32, feat_cnl=0, num_hidden=3, num_wide=64, short_cut=0, isglobal=0, optim_trans=0,
          optim_spatialvariant_trans=0, n_img=34, n_pattern=34, poses_per_image=0, H=400, W=400, kernel_hwindow=10.0, random_hwindow=0.25, fx=350.0, fy=350.0,
          cx=200.0, cy=200.0)


def _fwd(h, d, prm, R):
    return h.evd_sparse_blur_forward(C.byref(d), C.byref(prm), None, None, None, None, None, None, None, R, None, None, None, None, None, 0, None)


def _bwd(h, d, prm, R, grads=None):
    return h.evd_sparse_blur_backward(C.byref(d), C.byref(prm), None, None, None, None, None, None, None, R, None, None, None, None, grads, None, None, None, 0, None)


def test_entries_validate_before_touching_the_device():
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd import build
    build.build()
    h = L.lib()
    d = L.SparseBlurDesc(**OK)
    # 16 x 16 weight-gradient tiles: linears.0 4 x 3 + 4 (bias), linears.2 / .4 and linears1.0 4 x 4 + 4 each, linears1.2 4 + 1
    tiles = 16 + 3 * 20 + 5
    blocks = 128                                                      # 1024 rays in tiles of 16 // 5 = 3: 342 tiles on at most 128 workgroups
    assert h.evd_sparse_blur_workspace_bytes(C.byref(d), 1024) == 4 * (1024 * 32 + 4 * 1024 * 5 + blocks * tiles * 256)
    assert h.evd_sparse_blur_workspace_bytes(C.byref(d), 0) == 0
    prm = L.SparseBlurParams()
    assert _fwd(h, d, prm, 0) == 0                                    # R = 0: no-op
    assert h.evd_sparse_blur_workspace_bytes(C.byref(d), -1) == 0
    assert _fwd(h, d, prm, 8) == -1 and b"evd_sparse_blur_forward" in h.evd_last_error() and b"null" in h.evd_last_error()
    assert _bwd(h, d, prm, 8) == -1 and b"evd_sparse_blur_backward" in h.evd_last_error()
    assert _bwd(h, d, prm, 0) == -1 and b"null gradient buffer" in h.evd_last_error()
    assert h.evd_sparse_blur_forward(None, C.byref(prm), None, None, None, None, None, None, None, 8, None, None, None, None, None, 0, None) == -1
    assert b"null descriptor" in h.evd_last_error()
    for bad, word in ((dict(num_wide=65), b"num_wide"), (dict(num_wide=0), b"num_wide"), (dict(num_hidden=5), b"num_hidden"), (dict(num_hidden=0), b"num_hidden"),
                      (dict(embed_cnl=114), b"row width"), (dict(kernel_type=1, feat_cnl=64, spatial_embed=4), b"row width"), (dict(num_pt=17), b"num_pt"),
                      (dict(num_pt=0), b"num_pt"), (dict(in_embed=5), b"in_embed"), (dict(in_embed=0), b"in_embed"), (dict(spatial_embed=5), b"spatial_embed"),
                      (dict(spatial_embed=-1), b"spatial_embed")):
        db = L.SparseBlurDesc(**dict(OK, **bad))
        for call, who in ((_fwd, b"evd_sparse_blur_forward"), (_bwd, b"evd_sparse_blur_backward")):
            assert call(h, db, prm, 8) == -1
            msg = h.evd_last_error()
            assert who in msg and word in msg, msg
        assert h.evd_sparse_blur_workspace_bytes(C.byref(db), 8) == 0
    assert h.evd_sparse_blur_workspace_bytes(C.byref(L.SparseBlurDesc(**dict(OK, embed_cnl=113))), 8) > 0          # row width 127: the largest


def test_kernel_type_check_of_the_training_call():
    """what NeRFAll's training branches ask before they run a kernelsnet (the whole call with a model is in tests/test_gpu_sparse_blur.py):
    PBE needs the differentiable composite-feature coarse render"""
    from evdeblurnerf_amd.renderer import NeRFAll
    probe = SimpleNamespace(kernel_type="PBE")
    with pytest.raises(NotImplementedError, match="composite-feature coarse render"):
        NeRFAll._check_kernel_type(probe)
    for ok in ("RBK", "DSK"):
        NeRFAll._check_kernel_type(SimpleNamespace(kernel_type=ok))
    with pytest.raises(NotImplementedError, match="none"):
        NeRFAll._check_kernel_type(SimpleNamespace(kernel_type="none"))
