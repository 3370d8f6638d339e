"""CPU-only: the C ABI of the deterministic training mode (evd_voxel_sample_bwd_det, its workspace query, evd_scatter_det_unit_exp,
evd_crf_set_deterministic) is exported and bound, validates its arguments before touching the device, and the fixed-point scale the
scatter takes from evd_scatter_det_unit_exp cannot overflow a 64-bit accumulator.

The scale: with frexp(cmax) -> E (cmax < 2^E) and h = ceil(log2(4 n)), k = 62 - h - E and the unit is 2^-k.  A cell receives at most 4 n
contributions of magnitude <= cmax, so its sum is below 4 n cmax 2^k <= 2^62 units.  k is clamped to 126 (the clamp of k_scatter_lines: 2^k
must be a finite float32), so "40 bits below the batch maximum" (unit <= 2^(E - 40) for n <= 2^20) holds where E - 40 >= -126; a batch whose
maximum is below 2^-86 is resolved to 2^-126 instead -- both properties together cannot hold there (2^(E - 40) would need k > 127), and
2^-126 is the smallest normal float32, far below anything a float32 sum of such terms resolves."""
import ctypes
import math

import numpy as np
import pytest

NEW = ("evd_voxel_sample_bwd_det_workspace_bytes", "evd_voxel_sample_bwd_det", "evd_scatter_det_unit_exp", "evd_crf_set_deterministic")


@pytest.fixture(scope="module")
def lib():
    from evdeblurnerf_amd import build, _lib
    build.build()
    return _lib.lib()


def test_new_symbols_exported_and_bound(lib):
    from evdeblurnerf_amd import _lib
    from test_cabi_symbols import declared_symbols
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared_symbols(), f"{name} is not declared in include/evdnerf.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert set(_lib.SIGNATURES) == set(declared_symbols())


def test_argument_validation_without_gpu(lib):
    rc = lib.evd_voxel_sample_bwd_det(None, 0, None, 4, None, 32, 0, None, None, None, 0, None)
    assert rc == -1 and b"evd_voxel_sample_bwd_det" in lib.evd_last_error()
    assert lib.evd_voxel_sample_bwd_det_workspace_bytes(None, 1024) == 0
    rc = lib.evd_crf_set_deterministic(None, 1)
    assert rc == -1 and b"evd_crf_set_deterministic" in lib.evd_last_error()


CMAX = (2.0 ** -140, 2.0 ** -126, 2.0 ** -78, 1e-20, 1.0, 3e38)
NS = (1, 31, 2 ** 10, 2 ** 20, 2 ** 31 - 1)
K_CLAMP = 126


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cmax", CMAX, ids=[f"{c:.3g}" for c in CMAX])
def test_unit_exponent_cannot_overflow(lib, cmax, n):
    c32 = float(np.float32(cmax))
    assert c32 > 0
    k = lib.evd_scatter_det_unit_exp(c32, n)
    # the documented formula
    _, E = math.frexp(c32)
    h = math.ceil(math.log2(4 * n))
    assert k == min(62 - h - E, K_CLAMP)
    # no overflow: exact in Python's integers / fractions of powers of two
    from fractions import Fraction
    assert 4 * n * Fraction(c32) * Fraction(2) ** k < 2 ** 63
    # 2^k is a finite, normal float32
    up = np.float32(2.0) ** np.float32(k)
    assert np.isfinite(up) and float(up) == 2.0 ** k and -126 <= k <= 127
    # at least 40 bits below the batch maximum for n <= 2^20 -- where the clamp allows it (see the module docstring)
    if n <= 2 ** 20:
        if E - 40 >= -K_CLAMP:
            assert -k <= E - 40
        else:
            assert k == K_CLAMP


def test_unit_exponent_without_a_scale(lib):
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.evd_scatter_det_unit_exp(bad, 100) == 0
    assert lib.evd_scatter_det_unit_exp(1.0, 0) == 0
