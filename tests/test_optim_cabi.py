"""CPU-only: the optimizer entries validate their arguments before they touch the device (evd_adam_create is a host call; the step and
the norm check the tables, the groups and the workspace first), and the empty cases are no-ops that return EVD_OK."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from evdeblurnerf_amd import build, _lib
    build.build()
    _lib.lib()
    return _lib


P = lambda on=True, a=0x1000: C.c_void_p(a) if on else None       # pointers are dummies: a valid call is never made here


def segments(L, rows):
    segs = (L.AdamSegment * max(len(rows), 1))()
    for s, r in zip(segs, rows):
        s.param, s.exp_avg, s.exp_avg_sq, s.mirror_f32, s.mirror_f16, s.n, s.group, s.clip = r
    return segs


def create(L, rows, ngroups=2):
    h = C.c_void_p()
    rc = L.lib().evd_adam_create(segments(L, rows), len(rows), ngroups, C.byref(h))
    return rc, h


ROW = (0x1000, 0x2000, 0x3000, None, None, 10, 1, 1)


def groups(L, n=2):
    g = (L.AdamGroup * n)()
    for x in g:
        x.lr, x.beta1, x.beta2, x.eps, x.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 0.
    return g


def test_create_rejects_bad_tables(L):
    lib = L.lib()
    bad = [ROW[:5] + (-1, 0, 1), ROW[:5] + (10, 2, 1), ROW[:5] + (10, -1, 1), (None,) + ROW[1:], ROW[:1] + (None,) + ROW[2:], ROW[:2] + (None,) + ROW[3:],
           (0x1002,) + ROW[1:]]
    for row in bad:
        rc, h = create(L, [ROW, row])
        assert rc == -1 and not h.value, row
        assert b"evd_adam_create" in lib.evd_last_error(), row
    assert lib.evd_adam_create(None, 1, 1, C.byref(C.c_void_p())) == -1
    assert lib.evd_adam_create(segments(L, [ROW]), 1, 2, None) == -1
    assert create(L, [ROW], ngroups=0)[0] == -1 and create(L, [ROW], ngroups=1)[0] == -1          # (the row names group 1)
    rc, h = create(L, [ROW, (None, None, None, None, None, 0, 0, 0)])                             # a zero-length segment needs no arrays
    assert rc == 0 and h.value
    lib.evd_adam_destroy(h)
    lib.evd_adam_destroy(None)


def test_step_and_norm_reject_bad_arguments_before_the_device(L):
    lib = L.lib()
    rc, h = create(L, [ROW, ROW[:5] + (5000, 0, 0)])
    assert rc == 0
    need = lib.evd_adam_workspace_bytes(h)
    assert need >= 1024 * 8 + 2 * 16 and lib.evd_adam_workspace_bytes(None) == 0
    grads, steps, g = (C.c_void_p * 2)(0x4000, None), (C.c_long * 2)(0, 3), groups(L)
    step = lambda **kw: lib.evd_adam_step(kw.get("h", h), kw.get("grads", grads), kw.get("steps", steps), kw.get("groups", g), kw.get("ngroups", 2),
                                          kw.get("max_norm", 0.), kw.get("norm", None), 0, kw.get("ws", P()), kw.get("ws_bytes", need), None)
    cases = [dict(h=None), dict(grads=None), dict(steps=None), dict(groups=None), dict(ngroups=1), dict(ngroups=3), dict(max_norm=1.0),
             dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(grads=(C.c_void_p * 2)(0x4001, None)), dict(steps=(C.c_long * 2)(-1, 0))]
    for kw in cases:
        assert step(**kw) == -1, kw
        assert b"evd_adam_step" in lib.evd_last_error(), kw
    assert b"workspace" in (step(ws_bytes=need - 1), lib.evd_last_error())[1]
    norm = lambda **kw: lib.evd_grad_norm(kw.get("h", h), kw.get("grads", grads), kw.get("out", P()), kw.get("ws", P()), kw.get("ws_bytes", need), None)
    for kw in (dict(h=None), dict(grads=None), dict(out=None), dict(ws=None), dict(ws_bytes=need - 1)):
        assert norm(**kw) == -1, kw
        assert b"evd_grad_norm" in lib.evd_last_error(), kw
    lib.evd_adam_destroy(h)


def test_empty_tables_are_no_ops(L):
    lib = L.lib()
    g = groups(L, 1)
    rc, h = create(L, [], ngroups=1)                                # nseg == 0
    assert rc == 0 and lib.evd_adam_step(h, None, None, g, 1, 0., None, 0, None, 0, None) == 0
    lib.evd_adam_destroy(h)
    rc, h = create(L, [(0x1000, 0x2000, 0x3000, None, None, 0, 0, 1)] * 3, ngroups=1)         # all-zero-length segments
    grads, steps = (C.c_void_p * 3)(0x4000, 0x4000, None), (C.c_long * 3)(0, 0, 0)
    assert rc == 0 and lib.evd_adam_step(h, grads, steps, g, 1, 0., None, 1, None, 0, None) == 0
    lib.evd_adam_destroy(h)


def test_grid_mirrors_rejects_null(L):
    lib = L.lib()
    a = (C.c_void_p * 3)()
    assert lib.evd_voxel_grid_mirrors(None, a, a, C.byref(C.c_void_p()), a, a) == -1
    assert b"evd_voxel_grid_mirrors" in lib.evd_last_error()
