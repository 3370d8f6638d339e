"""The AWP sample embedding on float32 rows (evd_awp_embed_f32_*: input_ch 64 / 128 / 256, width 64, depth 1..8 -- the proposal of a
mode='nerf' model reads netwidth channels per sample, run_nerf.py:223) against a float64 MLP, reference networks/dpnerf/awp.py:98-100.

Shapes (input_ch, depth, n): (256, 4, 300), (64, 4, 33), (128, 2, 129): a partial 32-sample tile, a partial 128-sample workgroup, more
than one workgroup.  Inputs are post-ReLU-like (half of the entries zero), as the NeRF network's before_linear feature is.  A sample
with a float64 pre-activation within TAU = 2e-6 of zero has its ReLU decided by rounding: its d h_local row is zero (at most 10 % of a
shape's samples; with these seeds none).  Bounds: forward 2e-5 (the project's bound for float32-grade outputs; |h| <= ~1 here), gradients 5e-6
relative L2 (tests/test_gpu_nerf_generic_train.py)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_train import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(256, 4, 300), (64, 4, 33), (128, 2, 129)]
TAU, TIE_CAP = 2e-6, 0.10


def make_params(input_ch, depth, seed):
    """nn.Linear's default ranges: weights and biases uniform in +-1 / sqrt(fan_in)"""
    rs = np.random.RandomState(seed)
    ws, bs = [], []
    for l in range(depth):
        fan = input_ch if l == 0 else 64
        ws.append(rs.uniform(-1, 1, (64, fan)).astype(np.float32) / np.float32(np.sqrt(fan)))
        bs.append(rs.uniform(-1, 1, (64,)).astype(np.float32) / np.float32(np.sqrt(fan)))
    return ws, bs


def make_rows(input_ch, n, seed):
    return np.maximum(np.random.RandomState(seed).normal(size=(n, input_ch)), 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(input_ch, depth, n):
    """float64, computed once and shared: h_local, the d h_local used (tie rows zeroed), fraction of tie samples, gradients"""
    ws, bs = make_params(input_ch, depth, 70 + depth)
    x = torch.tensor(make_rows(input_ch, n, 80), dtype=torch.float64, requires_grad=True)
    pw = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    pb = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    h, ties = x, torch.zeros(n, dtype=torch.bool)
    for w, b in zip(pw, pb):
        pre = h @ w.T + b
        ties |= (pre.detach().abs() < TAU).any(-1)
        h = torch.relu(pre)
    d_h = np.random.RandomState(81).normal(size=(n, 64)).astype(np.float32)
    d_h[ties.numpy()] = 0.0
    (h * torch.tensor(d_h, dtype=torch.float64)).sum().backward()
    return dict(h=h.detach(), d_h=d_h, frac=float(ties.double().mean()), gw=[w.grad for w in pw], gb=[b.grad for b in pb], gx=x.grad)


def T(x):
    return torch.tensor(x, device=DEV)


def make_embed(input_ch, depth, precision="f16"):
    from evdeblurnerf_amd.awp import SampleFeatureEmbed
    ws, bs = make_params(input_ch, depth, 70 + depth)
    emb = SampleFeatureEmbed(ws, bs, precision)
    flat = torch.cat([T(t).reshape(-1) for w, b in zip(ws, bs) for t in (w, b)]).requires_grad_(True)
    return emb, flat


def run(input_ch, depth, n, precision="f16"):
    emb, flat = make_embed(input_ch, depth, precision)
    assert emb.generic
    x = T(make_rows(input_ch, n, 80)).requires_grad_(True)
    h = emb(flat, x)
    (h * T(reference(input_ch, depth, n)["d_h"])).sum().backward()
    return emb, h.detach(), flat.grad, x.grad


@pytest.mark.parametrize("input_ch,depth,n", SHAPES + [(128, 4, 40)])
def test_forward_and_backward_match_float64(input_ch, depth, n):
    """(128, 4, 40): the shape of the half-precision kernels, which precision='f32' sends down the float32 rows path"""
    prec = "f32" if (input_ch, depth) == (128, 4) else "f16"
    ref = reference(input_ch, depth, n)
    assert ref["frac"] <= TIE_CAP
    emb, h, gflat, gx = run(input_ch, depth, n, prec)
    err = (h.cpu().double() - ref["h"]).abs().max().item()
    errs = {"d_rows": rel_l2(gx.cpu().double(), ref["gx"])}
    for l, (wo, bo) in enumerate(emb.offsets):
        errs[f"{l}.weight"] = rel_l2(gflat[wo:bo].cpu().double().reshape(ref["gw"][l].shape), ref["gw"][l])
        errs[f"{l}.bias"] = rel_l2(gflat[bo:bo + 64].cpu().double(), ref["gb"][l])
    worst = max(errs, key=errs.get)
    print(f"[input_ch {input_ch}, depth {depth}, n {n}] max |h_local - float64| = {err:.2e} (max |h_local| = {ref['h'].abs().max().item():.2f}); worst gradient "
          f"{worst} {errs[worst]:.2e}; {100 * ref['frac']:.1f} % of the samples zeroed as ties")
    assert err < 2e-5
    assert errs[worst] < 5e-6, {k: f"{v:.1e}" for k, v in errs.items()}


@pytest.mark.parametrize("input_ch,depth,n", SHAPES)
def test_repeats_bit_for_bit(input_ch, depth, n):
    a, b = run(input_ch, depth, n), run(input_ch, depth, n)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert a[2].abs().max().item() > 0 and a[3].abs().max().item() > 0


def test_depth_range_and_refusals():
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.awp import SampleFeatureEmbed
    for depth in (1, 8):
        ref = reference(64, depth, 40)
        _, h, _, _ = run(64, depth, 40)
        assert (h.cpu().double() - ref["h"]).abs().max().item() < 2e-5
    for input_ch, width, depth in ((96, 64, 4), (64, 32, 4), (64, 64, 9)):
        rs = np.random.RandomState(1)
        ws = [rs.normal(size=(width, input_ch if l == 0 else width)).astype(np.float32) for l in range(depth)]
        with pytest.raises(L.EvdError):
            SampleFeatureEmbed(ws, [np.zeros(width, np.float32)] * depth)
    emb, flat = make_embed(64, 4)
    with pytest.raises(L.EvdError):
        emb(flat, torch.zeros((8, 128), device=DEV))


def test_default_shape_in_f16_is_unchanged():
    """(128, 64, 4) in f16: SampleFeatureEmbed still runs the fused half-precision kernel -- the same bits as that entry called directly"""
    from evdeblurnerf_amd import _lib as L
    emb, flat = make_embed(128, 4, "f16")
    assert not emb.generic
    n = 300
    x = T(make_rows(128, n, 80))
    with torch.no_grad():
        got = emb(flat, x)
    lib = L.lib()
    nb = int(lib.evd_awp_embed_store_bytes(emb._h, n))
    store = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    want = torch.empty((n, 64), dtype=torch.float32, device=DEV)
    L.check(lib.evd_awp_embed_forward(emb._h, L.PREC["f16"], L.ptr(x), None, None, 0, n, L.ptr(want), L.ptr(store), nb, L.stream_ptr()), "evd_awp_embed_forward")
    assert torch.equal(got, want)
    ref = reference(128, 4, n)
    err = (got.cpu().double() - ref["h"]).abs().max().item()
    print(f"[128 -> 64 x 4, f16] max |h_local - float64| = {err:.2e}: the half-precision kernel's error, not the float32 path's")
