"""CPU-only: evd_edi_prior validates its arguments before it touches the device, and evd_edi_prior_workspace_bytes is the figure the
header states (positive, growing with every argument up to the cap of 16 images per chunk)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from evdeblurnerf_amd import build, _lib
    build.build()
    return _lib.lib()


def call(h, events=1, coords=1, bounds=1, images=1, out=1, ws=1, n_img=1, steps=9, hh=4, w=6, ws_bytes=None, N=10, n_coords=5):
    """pointers are dummies (non-null = 0x1000): a valid call is never made here"""
    P = lambda on: C.c_void_p(0x1000) if on else None
    need = h.evd_edi_prior_workspace_bytes(1, steps, hh, w)
    return h.evd_edi_prior(P(events), N, P(coords), n_coords, P(bounds), P(images), n_img, steps, hh, w, 0.2, 0.25, P(out), None, None, P(ws),
                           need if ws_bytes is None else ws_bytes, None)


def test_null_pointers_are_rejected(lib):
    for kw in ({"events": 0}, {"coords": 0}, {"bounds": 0}, {"images": 0}, {"out": 0}, {"ws": 0}):
        assert call(lib, **kw) == -1, kw
        assert b"evd_edi_prior" in lib.evd_last_error(), kw


def test_steps_must_be_odd_and_at_least_3(lib):
    for steps in (8, 2, 1, 0, -3, 10):
        assert call(lib, steps=steps, ws_bytes=1 << 30) == -1, steps
        assert b"evd_edi_prior" in lib.evd_last_error() and b"steps" in lib.evd_last_error()


def test_sizes_must_be_positive(lib):
    for kw in ({"n_img": 0}, {"hh": 0}, {"w": 0}, {"N": -1}, {"n_coords": -1}, {"n_img": -2}):
        assert call(lib, ws_bytes=1 << 30, **kw) == -1, kw
        assert b"evd_edi_prior" in lib.evd_last_error(), kw


def test_workspace_one_byte_short_is_rejected(lib):
    need = lib.evd_edi_prior_workspace_bytes(1, 9, 4, 6)
    assert need >= 8 * 4 * 6 * 16
    assert call(lib, ws_bytes=need - 1) == -1
    msg = lib.evd_last_error()
    assert b"evd_edi_prior" in msg and b"workspace" in msg
    assert call(lib, n_img=5, ws_bytes=need - 1) == -1              # (one image's worth is the floor whatever n_img)


def test_workspace_bytes_positive_and_monotone_up_to_the_cap(lib):
    f = lib.evd_edi_prior_workspace_bytes
    base = f(1, 3, 1, 1)
    assert base > 0
    prev = 0
    for n in range(1, 17):                                          # grows up to 16 images per chunk, then stays
        v = f(n, 9, 260, 346)
        assert v > prev and v >= n * 8 * 260 * 346 * 16
        prev = v
    assert f(17, 9, 260, 346) == prev and f(1000, 9, 260, 346) == prev
    assert f(1, 9, 260, 346) < 12.1e6                               # 11.5 MB of planes per image at the DAVIS size
    for lo, hi in (((4, 3, 48, 64), (4, 5, 48, 64)), ((4, 9, 48, 64), (4, 9, 49, 64)), ((4, 9, 48, 64), (4, 9, 48, 65)), ((4, 63, 48, 64), (4, 65, 48, 64))):
        assert 0 < f(*lo) < f(*hi), (lo, hi)
    for bad in ((0, 9, 4, 4), (1, 8, 4, 4), (1, 67, 4, 4), (1, 9, 0, 4), (1, 9, 4, 0)):
        assert f(*bad) == 0, bad
