"""The feature merge of the c2f pass on the GPU, alone: evd_merge_features / evd_merge_features_bwd (k_merge_features, k_merge_features_bwd)
and renderer._MergeFeatures.  They are row copies, so everything is compared bit for bit: the reference is torch.gather on the CPU over
cat([old, fresh], 1) (renderer.py:209-213)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (R, S, N, F, Ff); lanes = R (S + N) F / 4: 2, 21, 5920 (= 23 x 256 + 32: a partial last block), 132096 (= 516 x 256)
CASES = [(1, 1, 1, 4, 0), (3, 5, 2, 4, 4), (37, 24, 16, 16, 32), (129, 64, 64, 32, 64)]
SENTINEL = -7.654321e8


assert any((R * (S + N) * F // 4) % 256 for R, S, N, F, _ in CASES)


def make_order(rs, R, S, N, kind):
    if kind == "random":
        return np.stack([rs.permutation(S + N) for _ in range(R)]).astype(np.int32)
    # what evd_sample_pdf_merge gives: the stable sort order of cat([z (sorted), z_samples (sorted)])
    z = np.concatenate([np.sort(rs.uniform(0, 1, (R, S)), -1), np.sort(rs.uniform(0, 1, (R, N)), -1)], -1)
    return np.argsort(z, -1, kind="stable").astype(np.int32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def inputs(R, S, N, F, Ff, kind):
    rs = np.random.RandomState(R * 1000 + S + (kind == "random"))
    old = torch.tensor(rs.standard_normal((R, S, F)).astype(np.float32))
    fresh = torch.tensor(rs.standard_normal((R, N, F)).astype(np.float32))
    order = torch.tensor(make_order(rs, R, S, N, kind))
    assert all(sorted(row.tolist()) == list(range(S + N)) for row in order)
    ref = torch.gather(torch.cat([old, fresh], 1), 1, order.long()[..., None].expand(R, S + N, F))
    return rs, old, fresh, order, ref


@pytest.mark.parametrize("kind", ["merge", "random"])
@pytest.mark.parametrize("R,S,N,F,Ff", CASES)
def test_forward_is_the_gather_and_leaves_the_fine_window_alone(R, S, N, F, Ff, kind):
    from evdeblurnerf_amd import _lib as L
    rs, old, fresh, order, ref = inputs(R, S, N, F, Ff, kind)
    fine = torch.tensor(rs.standard_normal((R, S + N, Ff)).astype(np.float32))
    host = torch.full((R, S + N, F + Ff), SENTINEL, dtype=torch.float32)
    host[..., F:] = fine
    out, d_old, d_fresh, d_order = host.cuda(), old.cuda(), fresh.cuda(), order.cuda()
    L.check(L.lib().evd_merge_features(L.ptr(d_old), L.ptr(d_fresh), L.ptr(d_order), R, S, N, F, L.ptr(out), F + Ff, L.stream_ptr()),
            "evd_merge_features")
    torch.cuda.synchronize()
    assert torch.equal(bits(out[..., :F]), bits(ref))
    assert torch.equal(bits(out[..., F:]), bits(fine))


@pytest.mark.parametrize("kind", ["merge", "random"])
@pytest.mark.parametrize("R,S,N,F,Ff", CASES)
def test_backward_writes_every_row_once_and_reads_no_fine_column(R, S, N, F, Ff, kind):
    from evdeblurnerf_amd import _lib as L
    rs, old, fresh, order, _ = inputs(R, S, N, F, Ff, kind)
    d_out = torch.tensor(rs.standard_normal((R, S + N, F + Ff)).astype(np.float32))
    # the permuted gradient rows: row order[r, k] of cat([d_old, d_fresh], 1) is d_out[r, k, :F]
    ref = torch.empty((R, S + N, F))
    ref.scatter_(1, order.long()[..., None].expand(R, S + N, F), d_out[..., :F].contiguous())
    dev_order = order.cuda()

    def run(g):
        d_old = torch.full((R, S, F), float("nan"), dtype=torch.float32, device="cuda")
        d_fresh = torch.full((R, N, F), float("nan"), dtype=torch.float32, device="cuda")
        dev_g = g.cuda()
        L.check(L.lib().evd_merge_features_bwd(L.ptr(dev_g), F + Ff, L.ptr(dev_order), R, S, N, F, L.ptr(d_old), L.ptr(d_fresh), L.stream_ptr()),
                "evd_merge_features_bwd")
        torch.cuda.synchronize()
        return torch.cat([d_old.cpu(), d_fresh.cpu()], 1)

    got = run(d_out)
    assert not bool(torch.isnan(got).any()), "a gradient row was never written"
    assert torch.equal(bits(got), bits(ref))
    other = d_out.clone()
    other[..., F:] = float("nan")
    assert torch.equal(bits(run(other)), bits(ref)), "the fine columns of d_out were read"


@pytest.mark.parametrize("kind", ["merge", "random"])
@pytest.mark.parametrize("R,S,N,F,Ff", [c for c in CASES if c[4] > 0])
def test_merge_features_function_placed_and_unplaced(R, S, N, F, Ff, kind):
    from evdeblurnerf_amd.renderer import _MergeFeatures, _window
    rs, old, fresh, order, ref = inputs(R, S, N, F, Ff, kind)
    fine = torch.tensor(rs.standard_normal((R, S + N, Ff)).astype(np.float32))
    g = torch.tensor(rs.standard_normal((R, S + N, F + Ff)).astype(np.float32))
    d_ref = torch.empty((R, S + N, F))
    d_ref.scatter_(1, order.long()[..., None].expand(R, S + N, F), g[..., :F].contiguous())
    outs = []
    for placed in (False, True):
        ft0, ftn = old.cuda().requires_grad_(True), fresh.cuda().requires_grad_(True)
        if placed:
            rows = torch.full((R, S + N, F + Ff), SENTINEL, dtype=torch.float32, device="cuda")
            ft_fine = _window(rows, F, Ff)
            ft_fine.copy_(fine)                       # the fine gather has written its window
            ft_fine.requires_grad_(True)
            out = _MergeFeatures.apply(ft0, ftn, order.cuda(), ft_fine, rows)
            assert out.data_ptr() == rows.data_ptr()
        else:
            ft_fine = fine.cuda().requires_grad_(True)
            out = _MergeFeatures.apply(ft0, ftn, order.cuda(), ft_fine)
        assert torch.equal(bits(out[..., :F]), bits(ref)) and torch.equal(bits(out[..., F:]), bits(fine))
        out.backward(g.cuda())
        assert torch.equal(bits(ft_fine.grad), bits(g[..., F:]))
        assert torch.equal(bits(torch.cat([ft0.grad, ftn.grad], 1)), bits(d_ref))
        outs.append(out.detach().clone())
    assert torch.equal(bits(outs[0]), bits(outs[1]))


def test_invalid_arguments_are_errors():
    from evdeblurnerf_amd import _lib as L
    h = L.lib()
    R, S, N, F = 2, 3, 2, 8
    old, fresh = torch.zeros((R, S, F), device="cuda"), torch.zeros((R, N, F), device="cuda")
    order = torch.arange(S + N, dtype=torch.int32, device="cuda").repeat(R, 1)
    out = torch.full((R, S + N, F), SENTINEL, device="cuda")
    st = L.stream_ptr()
    good = lambda **kw: dict(dict(old=L.ptr(old), fresh=L.ptr(fresh), order=L.ptr(order), F=F, out=L.ptr(out), stride=F), **kw)
    fwd = lambda a: h.evd_merge_features(a["old"], a["fresh"], a["order"], R, S, N, a["F"], a["out"], a["stride"], st)
    bwd = lambda a: h.evd_merge_features_bwd(a["out"], a["stride"], a["order"], R, S, N, a["F"], a["old"], a["fresh"], st)
    for call, name in ((fwd, b"evd_merge_features"), (bwd, b"evd_merge_features_bwd")):
        for bad in (dict(F=6, stride=8), dict(stride=F - 4), dict(old=None), dict(fresh=None), dict(order=None), dict(out=None)):
            assert call(good(**bad)) != 0, (name, bad)
            assert name in h.evd_last_error()
        assert call(good()) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())           # the valid forward call wrote every row (the backward then read it)
