"""evd_voxel_mlp, the inference entry of the per-sample PDRF networks that the generic levels are tested through: exported, in the ctypes
table, and refusing a NULL level before it touches the device.  CPU only."""
import ctypes as C

from evdeblurnerf_amd import _lib as L


def test_evd_voxel_mlp_is_exported_and_refuses_a_null_level():
    assert "evd_voxel_mlp" in L.SIGNATURES
    fn = L.lib().evd_voxel_mlp
    buf = (C.c_float * 16)()
    rc = fn(None, L.PREC["f32"], buf, buf, 3, buf, 16, 1, 1, buf, None, None)
    assert rc != 0 and b"null argument" in L.lib().evd_last_error()
    assert list(buf) == [0.0] * 16


def test_backward_workspace_query_of_a_net_is_exported_and_answers_zero_for_a_null_level():
    """evd_voxel_backward_workspace_bytes_net: in the header's table, exported, 0 for a NULL handle in every precision (no device call:
    this test runs without a GPU); the handle-free query it equals on a standard level keeps its value (tests/test_workspace_sizes_cabi.py)"""
    assert L.SIGNATURES["evd_voxel_backward_workspace_bytes_net"][0] is C.c_size_t
    fn = L.lib().evd_voxel_backward_workspace_bytes_net
    assert [fn(None, p) for p in sorted(set(L.PREC.values()))] == [0] * len(set(L.PREC.values()))
    assert L.lib().evd_voxel_backward_workspace_bytes() > 0
