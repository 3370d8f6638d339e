"""CPU-only: the *_workspace_bytes queries that need neither a handle nor a device return, byte for byte, what they returned before each
entry got one layout function for its size query and its carve (csrc/evd_common.h Workspace).  The expected numbers are literals recorded
from the library as it was built from the commit before that change, not figures derived from the layouts under test."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from evdeblurnerf_amd import build, _lib
    build.build()
    _lib.lib()
    return _lib


# evd_nerf_render_workspace_bytes[(N_samples, N_importance)] = values at R = 0, 1, 3, 7, 1000 (the odd R: slot sizes that are no multiple of 256)
RENDER_R = (0, 1, 3, 7, 1000)
RENDER = {
    (3, 0): (256, 2048, 2048, 2560, 144640),
    (3, 4): (256, 2048, 2304, 3072, 252928),
    (3, 64): (256, 3584, 7168, 14848, 1932544),
    (8, 0): (256, 2048, 2304, 3072, 304384),
    (8, 4): (256, 2048, 2560, 4096, 412672),
    (8, 64): (256, 3584, 7424, 15360, 2092288),
    (64, 0): (256, 2816, 6912, 15360, 2096384),
    (64, 4): (256, 3584, 7680, 16384, 2204672),
    (64, 64): (256, 4352, 12032, 27648, 3884288),
}
BACKWARD = {"evd_nerf_backward_workspace_bytes": 75497984, "evd_voxel_backward_workspace_bytes": 75497984,
            "evd_awp_embed_backward_workspace_bytes": 13632000}
COLOR_MAP = {-1: 0, 0: 1024, 1: 1024, 255: 1792, 256: 1792, 257: 2304}
# evd_edi_prior_workspace_bytes: the argument rows of tests/test_edi_prior_cabi.py, and n_img above the chunk cap of 16 images
EDI = {
    (1, 3, 1, 1): 800, (1, 9, 4, 6): 3840, (4, 3, 48, 64): 393984, (4, 5, 48, 64): 787200, (4, 9, 48, 64): 1574144, (4, 9, 49, 64): 1606912,
    (4, 9, 48, 65): 1598720, (4, 63, 48, 64): 12194048, (4, 65, 48, 64): 12587776,
    (0, 9, 4, 4): 0, (1, 8, 4, 4): 0, (1, 67, 4, 4): 0, (1, 9, 0, 4): 0, (1, 9, 4, 0): 0,
    (1000, 9, 260, 346): 184240896, (3, 3, 2, 3): 1344, (16, 3, 2, 3): 4352, (17, 3, 2, 3): 4352, (40, 3, 2, 3): 4352,
}
EDI_DAVIS = (11515648, 23030528, 34545408, 46060800, 57575680, 69090560, 80605440, 92120832, 103635712, 115150592, 126665984, 138180864,
             149695744, 161210624, 172726016, 184240896, 184240896)      # (n_img, 9, 260, 346) for n_img = 1 .. 17

def render_bytes(L, S, Ni, R):
    cfg = L.RenderCfg()
    cfg.N_samples, cfg.N_importance, cfg.use_viewdirs = S, Ni, 1
    return L.lib().evd_nerf_render_workspace_bytes(C.byref(cfg), R)


def test_nerf_render_workspace_bytes(L):
    for (S, Ni), want in RENDER.items():
        assert tuple(render_bytes(L, S, Ni, R) for R in RENDER_R) == want, (S, Ni)
    assert L.lib().evd_nerf_render_workspace_bytes(None, 7) == 0
    assert render_bytes(L, 8, 4, -1) == 0 and render_bytes(L, 64, 64, -1000) == 0


def test_backward_workspace_bytes(L):
    for name, want in BACKWARD.items():
        assert getattr(L.lib(), name)() == want, name


def test_event_color_map_workspace_bytes(L):
    for n, want in COLOR_MAP.items():
        assert L.lib().evd_event_color_map_workspace_bytes(n) == want, n


def test_edi_prior_workspace_bytes(L):
    for args, want in EDI.items():
        assert L.lib().evd_edi_prior_workspace_bytes(*args) == want, args
    assert tuple(L.lib().evd_edi_prior_workspace_bytes(n, 9, 260, 346) for n in range(1, 18)) == EDI_DAVIS
