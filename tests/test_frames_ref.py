"""CPU-only.  (1) tests/frames_ref.py, the NumPy restatement the GPU pictures are compared with byte for byte
(tests/test_gpu_frames.py), against facts that do not depend on it: the float32 operation order of np.mean(-1) that the device kernel
spells out, and the two stated conventions (constant slice, NaN).  (2) The evd_frame_* entries reject bad arguments before they touch the
device, and evdeblurnerf_amd.frames rejects what it cannot run, with EvdError."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_ref as R


def test_mean_of_three_is_left_to_right_float32():
    """np.mean(-1) of a float32 [..., 3] array == ((a0 + a1) + a2) / float32(3) bit for bit; it is neither a0 + (a1 + a2) nor a float64 mean"""
    rs = np.random.RandomState(7)
    a = (rs.uniform(-0.2, 1.3, (40000, 3)) * 10.0 ** rs.randint(-6, 3, (40000, 1))).astype(np.float32)
    sq = a ** 2
    got = sq.mean(-1)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), R.mean3_explicit(sq).view(np.uint32))
    right = (sq[:, 0] + (sq[:, 1] + sq[:, 2])) / np.float32(3)
    wide = sq.astype(np.float64).mean(-1).astype(np.float32)
    assert (got != right).any() and (got != wide).any()            # the order is not a formality
    rgb, gt = a, a[::-1].copy()
    assert np.array_equal(R.pixmse(rgb, gt).view(np.uint32), R.mean3_explicit((rgb - gt) * (rgb - gt)).view(np.uint32))


def test_to8b_truncates_and_clips():
    x = np.array([-1.0, 0.0, 0.999 / 255, 1.5 / 255, 0.5, 254.999 / 255, 1.0, 7.0, np.nan, np.inf, -np.inf], np.float32)
    assert R.to8b(x).tolist() == [0, 0, 0, 1, 127, 254, 255, 255, 0, 255, 0]


def test_constant_slice_convention():
    """the divisor is 0: grey level 0 for the whole slice (through a table: its row 255).  A constant slice whose divisor is not 0 is
    defined in the reference -- every value / max == 1 -- and stays 255."""
    lut = np.random.RandomState(1).permutation(256 * 3).reshape(256, 3).astype(np.uint8)
    ones = np.ones((2, 3, 4), np.float32)
    assert not R.depth_images(ones, invert=True, scope="frame").any() and not R.depth_images(ones, invert=True, scope="all").any()
    assert not R.depth_images(0 * ones, invert=False, scope="frame").any()
    assert (R.depth_images(ones, invert=True, scope="frame", lut=lut) == lut[255]).all()
    assert (R.depth_images(0.25 * ones, invert=False, scope="frame") == 255).all()
    mixed = np.stack([np.ones((3, 4), np.float32), np.linspace(0, 0.5, 12, dtype=np.float32).reshape(3, 4)])      # a constant frame among others
    g = R.depth_images(mixed, invert=True, scope="frame")
    assert not g[0].any() and g[1].max() == 255
    rgb = np.random.RandomState(2).rand(2, 3, 4, 3).astype(np.float32)
    gt = rgb.copy()
    gt[1, 0, 0, 0] += 0.5
    e = R.error_maps(rgb, gt)
    assert not e[0].any() and e[1, 0, 0] == 255 and e[1].sum() == 255
    assert not R.video_frames(np.full((2, 3, 4, 3), 0.7, np.float32)).any()


def test_nan_convention():
    """a NaN value is grey level 0 and leaves every other byte where it would be without it"""
    rs = np.random.RandomState(3)
    d = rs.uniform(-0.2, 1.3, (2, 5, 7)).astype(np.float32)
    bad = d.copy()
    bad[1, 2, 3] = np.nan
    clean = d.copy()
    clean[1, 2, 3] = np.sort(d[1].ravel())[d[1].size // 2]          # a value that changes no maximum, inverted or not
    for scope in ("all", "frame"):
        for invert in (False, True):
            g, want = R.depth_images(bad, invert, scope), R.depth_images(clean, invert, scope)
            assert g[1, 2, 3] == 0
            want[1, 2, 3] = 0
            assert np.array_equal(g, want)
    rgb = rs.rand(2, 5, 7, 3).astype(np.float32)
    v = R.video_frames(np.where(np.arange(rgb.size).reshape(rgb.shape) == 17, np.nan, rgb).astype(np.float32))
    assert v.reshape(-1)[17] == 0 and v.max() == 255


# ------------------------------------------------------------------------------------------------ the C entries, without a device
@pytest.fixture(scope="module")
def lib():
    from evdeblurnerf_amd import _lib, build
    build.build()
    return _lib.lib()


P = C.c_void_p(0x1000)          # never dereferenced: every call below is rejected first


def test_frame_entries_reject_bad_arguments(lib):
    ws = lib.evd_frame_workspace_bytes
    assert ws(3, 1961, 0) >= 2 * 4 and ws(3, 1961, 1) >= 3 * 2 * 4
    assert ws(5, 129 * 131, 1) >= 5 * 3 * 2 * 4          # a 16899-value frame is more than one workgroup's share
    assert ws(0, 10, 0) == 0 and ws(3, 0, 0) == 0 and ws(-1, 10, 1) == 0 and ws(3, -5, 1) == 0 and ws(3, 10, 2) == 0 and ws(1 << 20, 1 << 30, 0) == 0
    need = ws(3, 1961, 1)

    def rng(x=P, y=None, source=0, scope=1, n=3, per=1961, out=P, w=P, wb=need):
        return lib.evd_frame_range(x, y, source, scope, n, per, out, w, wb, None)

    def mp(x=P, y=None, source=0, scope=1, n=3, per=1961, r=P, sub=0, lut=None, out=P):
        return lib.evd_frame_map(x, y, source, scope, n, per, r, sub, lut, out, None)

    for kw in (dict(x=None), dict(out=None), dict(source=2, y=None), dict(source=3), dict(source=-1), dict(scope=2), dict(scope=-1), dict(n=0), dict(n=-2),
               dict(per=0), dict(per=-7), dict(w=None), dict(wb=need - 1), dict(wb=0), dict(n=1 << 20, per=1 << 30)):
        assert rng(**kw) == -1, kw
        assert b"evd_frame_range" in lib.evd_last_error(), kw
    for kw in (dict(x=None), dict(out=None), dict(r=None), dict(source=2, y=None), dict(source=3), dict(scope=5), dict(n=0), dict(per=0), dict(per=-1),
               dict(n=1 << 20, per=1 << 30)):
        assert mp(**kw) == -1, kw
        assert b"evd_frame_map" in lib.evd_last_error(), kw
    assert lib.evd_frame_colormap(None, 5, P, P, None) == -1 and b"evd_frame_colormap" in lib.evd_last_error()
    assert lib.evd_frame_colormap(P, 5, None, P, None) == -1 and lib.evd_frame_colormap(P, 5, P, None, None) == -1
    assert lib.evd_frame_colormap(P, -1, P, P, None) == -1
    assert lib.evd_frame_colormap(None, 0, None, None, None) == 0                      # nothing to do: no launch


def test_frames_module_rejects_what_it_cannot_run(lib):
    from evdeblurnerf_amd import frames as F
    from evdeblurnerf_amd._lib import EvdError
    d, rgb = torch.rand(2, 5, 7), torch.rand(2, 5, 7, 3)
    lut = torch.arange(768, dtype=torch.int64).reshape(256, 3).to(torch.uint8)
    for call in (lambda: F.depth_images(d), lambda: F.depth_images(d, colormap=lut), lambda: F.error_maps(rgb, rgb), lambda: F.video_frames(rgb),
                 lambda: F.apply_colormap(torch.zeros(4, dtype=torch.uint8), lut)):
        with pytest.raises(EvdError, match="no CPU fallback"):
            call()
    for bad in (lut[:255], lut.to(torch.int32), lut.t().contiguous(), np.zeros((256, 4), np.uint8), lut.float()):
        with pytest.raises(EvdError, match="colour map"):
            F.depth_images(d, colormap=bad)
        with pytest.raises(EvdError, match="colour map"):
            F.error_maps(rgb, rgb, colormap=bad)
        with pytest.raises(EvdError, match="colour map"):
            F.apply_colormap(torch.zeros(4, dtype=torch.uint8), bad)
    with pytest.raises(EvdError, match="shapes must match"):
        F.error_maps(rgb, rgb[:1])
    with pytest.raises(EvdError, match="shapes must match"):
        F.error_maps(rgb, torch.rand(2, 5, 8, 3))
    with pytest.raises(EvdError, match="end in 3"):
        F.error_maps(d, d)
    with pytest.raises(EvdError, match="scope"):
        F.depth_images(d, scope="batch")
    with pytest.raises(EvdError, match="uint8 picture"):
        F.apply_colormap(torch.zeros(4), lut)
