"""CPU-only: the size queries of the AWP tail (evd_awp_tail_num_params / _param_count / _saved_floats) return what they returned before
kernel_awp_tail.hip was split (csrc/awp_tail.h).  evd_awp_tail_saved_floats is the row width of the saved_rays tensor that the forward
writes and the backward reads, and evd_awp_tail_param_count the length of d_params: both follow from tail_lds_layout / tail_param_size, and
an accidental reorder or resize there changes them.  The expected numbers are literals recorded from the library as it was built from the
commit before the split, not figures derived from the code under test."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from evdeblurnerf_amd import build, _lib
    build.build()
    _lib.lib()
    return _lib


NUM_PARAMS = {1: 14, 2: 16, 3: 18, 4: 20}
# (P, S, VF, dir_freqs, n_mot) -> (evd_awp_tail_param_count, evd_awp_tail_saved_floats)
SIZES = {
    (10, 128, 32, 2, 2): (10186, 13800),          # the shipped shape
    (5, 64, 4, 2, 3): (10181, 6580),
    (16, 40, 0, 2, 2): (9360, 9208),
    (6, 48, 22, -1, 2): (9254, 5696),             # no direction encoding in the kernel
    (2, 1, 0, 2, 1): (7842, 724),
}


def desc(L, P, S, VF, F, n_mot):
    return L.AwpTailDesc(P=P, S=S, VF=VF, dir_freqs=F, n_mot=n_mot, training=1, bn_eps=1e-5, bn_momentum=0.1)


def test_num_params(L):
    for n_mot, want in NUM_PARAMS.items():
        assert L.lib().evd_awp_tail_num_params(n_mot) == want, n_mot


def test_param_count_and_saved_floats(L):
    lib = L.lib()
    for key, (count, saved) in SIZES.items():
        d = desc(L, *key)
        assert lib.evd_awp_tail_param_count(C.byref(d)) == count, key
        assert lib.evd_awp_tail_saved_floats(C.byref(d)) == saved, key


def test_bad_descriptors(L):
    lib = L.lib()
    assert lib.evd_awp_tail_param_count(None) == -1 and lib.evd_awp_tail_saved_floats(None) == -1
    for key in ((10, 128, 32, 2, 0), (17, 128, 32, 2, 2)):          # no motion layer; more sub-exposures than the kernels are built for
        d = desc(L, *key)
        assert lib.evd_awp_tail_param_count(C.byref(d)) == -1, key
        assert lib.evd_awp_tail_saved_floats(C.byref(d)) == -1, key
