"""Pins the float64 compositing / resampling reference of tests/test_gpu_composite.py (tests/composite_ref.py) before any kernel is held
to it: to the goldens the real reference computed (G3, G4, G5) at their existing tolerances, to the CPU oracle's sample_pdf on the same
float32 knots, and its hand-written backward to torch float64 autograd.  CPU only."""
import numpy as np
import pytest
import torch

from composite_ref import composite, composite_autograd, composite_bwd, cdf_knots, linspace32, sample_pdf, sample_pdf_merge
from conftest import load_golden, maxabs, sample_pdf_flip_report
from oracle import oracle as O

U = 2.0 ** -24
G3_CASES = {"plain": {}, "white": dict(white=True), "rmnear": dict(rmnear=20 / 128), "relu_rgb": dict(rgb_act="relu"),
            "none_rgb": dict(rgb_act="none"), "softplus": dict(sigma_act="softplus")}


@pytest.mark.parametrize("eps", [0.0, 1e-10])
@pytest.mark.parametrize("S", [64, 128, 33])
def test_G3_with_and_without_the_reference_stabiliser(S, eps):
    g = load_golden("G3_nerf_raw2outputs")
    raw, z, d = torch.tensor(g[f"raw_S{S}"]), g[f"z_S{S}"], g[f"d_S{S}"]
    for tag, kw in G3_CASES.items():
        o = composite(raw, z, d, eps=eps, **kw)
        for k in ("rgb", "acc", "depth", "weights"):
            assert maxabs(o[k].numpy(), g[f"{k}_S{S}_{tag}"]) < 5e-6, (tag, k)
        if tag == "plain":
            assert maxabs(o["density"].numpy(), g[f"density_S{S}"]) < 5e-6
    o = composite(raw, z, d, feature=g[f"feat_S{S}"], eps=eps)
    assert maxabs(o["fmap"].numpy(), g[f"fmap_S{S}"]) < 5e-6


@pytest.mark.parametrize("S", [64, 128])
def test_G4_voxel_layouts_and_the_15_channel_map(S):
    g = load_golden("G4_voxel_raw2outputs")
    raw, z, d = torch.tensor(g[f"raw_S{S}"]), g[f"z_S{S}"], g[f"d_S{S}"]
    for tag, act in (("coarse", "relu"), ("fine", "none")):
        o = composite(raw, z, d, sigma_ch=0, rgb_ch0=1, rgb_act=act, form_name="il")
        for k in ("rgb", "acc", "depth", "weights"):
            assert maxabs(o[k].numpy(), g[f"{k}_S{S}_{tag}"]) < 5e-6, (tag, k)
    o = composite(torch.tensor(g[f"raw16_S{S}"]), z, d, sigma_ch=0, rgb_ch0=1, n_rgb=15, rgb_act="relu", form_name="weighted")
    assert maxabs(o["rgb"].numpy(), g[f"fmap16_S{S}"]) < 5e-6


def test_the_stabiliser_is_not_a_no_op_behind_an_opaque_sample_and_stays_within_S_1e_10():
    """the reference's + 1e-10 (nerf.py:116): behind a sample with alpha == 1 to float32 precision the transmittance is ~1e-10, not ~0; the
    difference on every output is at most S * 1e-10 (times the largest colour / depth)"""
    rs = np.random.RandomState(4)
    R, S = 16, 64
    raw = torch.tensor(rs.standard_normal((R, S, 4)))
    raw[:, 5, 3] = 1e9                                                        # opaque at sample 5
    z = np.sort(rs.uniform(1, 2, (R, S)), -1)
    d = rs.standard_normal((R, 3))
    a, b = composite(raw, z, d), composite(raw, z, d, eps=1e-10)
    assert float(a["scan"]["T"][:, 6].max()) < 1e-30 and float(b["scan"]["T"][:, 6].min()) > 5e-11
    for k, scale in (("weights", 1), ("acc", 1), ("depth", 2), ("rgb", 1)):
        assert float((a[k] - b[k]).abs().max()) <= S * 1e-10 * scale * 1.01, k


@pytest.mark.parametrize("S,N", [(64, 64), (64, 128), (128, 64), (17, 9)])
def test_G5_sample_pdf_matches_the_golden_and_the_oracle(S, N):
    """against the golden at its existing tolerance (sample_pdf_flip_report), and against the C oracle, which computes the same float32
    knots and index: there, element by element within 2 u of the bound"""
    g = load_golden("G5_sample_pdf")
    key = f"S{S}_N{N}"
    bins, w, u = g[f"bins_{key}"], g[f"w_{key}"], g[f"u_{key}"]
    R = bins.shape[0]
    ulin = linspace32(N)
    for name, uu, det in (("det", np.broadcast_to(ulin, (R, N)), True), ("rand", u, False)):
        s, E, _ = sample_pdf(bins, w, np.ascontiguousarray(uu))
        s = s.numpy()
        nbad, unexplained = sample_pdf_flip_report(s, g[f"{name}_{key}"], bins, w, ulin if det else u)
        assert unexplained == 0 and nbad <= 0.01 * s.size, (name, nbad, unexplained)
        o = O.sample_pdf(bins, w, N, det=det, u=None if det else u).astype(np.float64)
        assert (np.abs(o - s) <= 2 * U * E.numpy()).all(), (name, float(np.max(np.abs(o - s) / (U * E.numpy()))))


def test_sample_pdf_knots_index_and_guard_on_edges():
    """u exactly on a knot and one float32 ulp either side, u = 0 and 1, S = 3 (one weight), all-zero / one-hot / 1e-30 weights and
    duplicate z, against the oracle: the same index, samples within the bound"""
    rs = np.random.RandomState(8)
    for S in (3, 4, 17, 65):
        R = 12
        z = np.sort(rs.uniform(0, 4, (R, S)).astype(np.float32), -1)
        z[1, S // 2] = z[1, S // 2 - 1]                                            # duplicate z
        w = rs.uniform(0, 1, (R, S)).astype(np.float32)
        w[2] = 0
        w[3] = 0
        w[3, S // 2] = 1                                                           # one-hot
        w[4] *= np.float32(1e-30)
        knots = cdf_knots(torch.tensor(w[:, 1:-1])).numpy()
        cols = [np.zeros(R, np.float32), np.ones(R, np.float32)]
        for k in range(knots.shape[1]):
            c = knots[:, k]
            cols += [c, np.nextafter(c, np.float32(-1)), np.nextafter(c, np.float32(2))]
        u = np.clip(np.stack(cols, 1), 0, 1).astype(np.float32)
        r = sample_pdf_merge(z, w, u.shape[1], det=False, u=u)
        bins = (np.float32(0.5) * (z[:, 1:] + z[:, :-1])).astype(np.float32)
        o = O.sample_pdf(bins, w[:, 1:-1], u.shape[1], det=False, u=u).astype(np.float64)
        s, E = r["z_samples"].numpy(), r["E_z_samples"].numpy()
        assert (np.abs(o - s) <= 2 * U * E).all(), S
        # the index is searchsorted(right=True) on the float32 knots: u on a knot goes to the bin above it
        inds = r["inds"].numpy()
        assert (inds == np.stack([np.searchsorted(knots[i], u[i], side="right") for i in range(R)])).all()


@pytest.mark.parametrize("layout", ["nerf", "pdrf"])
def test_backward_matches_float64_autograd(layout):
    """the hand-written float64 backward against torch autograd of the plain forward, for every activation on either channel, white
    background, rmnear, noise, each upstream gradient None on its own"""
    rs = np.random.RandomState(3)
    R, S = 9, 37
    sc, c0 = (3, 0) if layout == "nerf" else (0, 1)
    cases = [dict(rgb_act=a) for a in ("sigmoid", "relu", "none", "exp", "sigmoid1", "softplus", "tanh")]
    cases += [dict(sigma_act=a) for a in ("softplus", "exp", "sigmoid", "sigmoid1", "none", "tanh")]
    cases += [dict(white=True), dict(rmnear=1.5), dict(noise=rs.standard_normal((R, S - 1)))]
    for kw in cases:
        raw = torch.tensor(rs.standard_normal((R, S, 4)))
        raw[..., sc] *= 3
        raw[0, :, sc] = 0.0
        raw[1, 3, sc] = 40.0 if kw.get("sigma_act") == "exp" else 1e3          # opaque
        z = np.sort(rs.uniform(1, 2, (R, S)), -1)
        z[2, 5] = z[2, 4]
        d = torch.tensor(rs.standard_normal((R, 3)))
        gs = [rs.standard_normal(sh) for sh in ((R, 3), (R,), (R,), (R, S))]
        for drop in (None, 0, 1, 2, 3):
            g = [None if i == drop else gs[i] for i in range(4)]
            ra, da = raw.clone().requires_grad_(True), d.clone().requires_grad_(True)
            rgb, acc, w, depth = composite_autograd(ra, z, da, sigma_ch=sc, rgb_ch0=c0, **kw)
            loss = sum((o * torch.tensor(gg)).sum() for o, gg in zip((rgb, depth, acc, w), g) if gg is not None)
            loss.backward()
            r = composite_bwd(raw, z, d, *g, sigma_ch=sc, rgb_ch0=c0, **kw)
            for got, ref, m in ((r["d_raw"], ra.grad, r["E_d_raw"]), (r["d_rays_d"], da.grad, r["E_d_rays_d"])):
                assert ((got - ref).abs() <= 1e-9 * (m + ref.abs())).all(), (kw, drop, float((got - ref).abs().max()))


def test_the_white_background_term_has_no_gradient():
    """rgb + (1 - acc): acc = 1 - prod(1 - alpha) = 1 exactly (the last alpha is 1), so the white background adds nothing to d raw or
    d rays_d; the backward's `- sum g_map` term in G_i only changes rounding"""
    rs = np.random.RandomState(6)
    R, S = 7, 40
    raw = torch.tensor(rs.standard_normal((R, S, 4)) * [1, 1, 1, 5])
    z = np.sort(rs.uniform(1, 2, (R, S)), -1)
    d = torch.tensor(rs.standard_normal((R, 3)))
    g = [rs.standard_normal(sh) for sh in ((R, 3), (R,), (R,), (R, S))]
    a, b = composite_bwd(raw, z, d, *g, white=True), composite_bwd(raw, z, d, *g, white=False)
    for k in ("d_raw", "d_rays_d"):
        assert ((a[k] - b[k]).abs() <= 1e-12 * (a["E_" + k] + 1)).all(), k
