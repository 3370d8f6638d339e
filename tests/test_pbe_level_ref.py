"""CPU-only: the float64 references of tests/pbe_level_ref.py (feature-composite backward, per-ray colour network) against float64
autograd of plain-torch restatements and against the reference's golden G25, the input conditions of every GPU case, and -- without
running a kernel -- that each structural fault changes some output by more than the bound the GPU test allows there."""
import numpy as np
import pytest
import torch

import pbe_level_ref as P
import voxel_level_ref as V
from conftest import load_golden
from evdeblurnerf_amd import weights as W

U, K = 2.0 ** -24, 2.0


def _t(v):
    return None if v is None else torch.as_tensor(v)


@pytest.mark.parametrize("c", P.FEAT_CASES, ids=[c["id"] for c in P.FEAT_CASES])
def test_feature_composite_backward_is_autograd(c):
    a = P.feat_inputs(c)
    r = P.feat_reference(c)
    sg, rows = _t(a["raw"][..., 0]).double().requires_grad_(True), _t(a["rows"]).double().requires_grad_(True)
    rd = _t(a["rays"][:, a["col"]:a["col"] + 3]).double().requires_grad_(True)
    outs = P.feat_composite_autograd(sg, rows, a["z"], rd, rows_act=c["act"], noise=a["noise"])
    loss = sum((o * _t(g).double()).sum() for o, g in zip((outs[0], outs[3], outs[1], outs[2]), a["g"]) if g is not None)
    gs = torch.autograd.grad(loss, (sg, rows, rd), allow_unused=True)
    for name, g in zip(("d_sigma", "d_rows", "d_rays_d"), gs):
        g = torch.zeros_like(r[name]) if g is None else g
        assert float((g - r[name]).abs().max()) <= 1e-12 * max(1.0, float(r[name].abs().max())), name
    if c["S"] == 1:
        assert not r["d_sigma"].any()                       # only the forced-alpha sample
    assert (r["d_sigma"][:, -1] == 0).all()


@pytest.mark.parametrize("c", P.FEAT_CASES, ids=[c["id"] for c in P.FEAT_CASES])
def test_feature_composite_input_condition(c):
    rows = P.feat_inputs(c)["rows"]
    pos = float((rows > 0).mean())
    assert 0.25 <= pos <= 0.75, pos
    r = P.feat_reference(c)
    for k in ("d_sigma", "d_rows", "d_rays_d"):
        assert torch.isfinite(r[k]).all() and torch.isfinite(r["E_" + k]).all(), k


def _exceeds(ref, bad, names):
    """some element of some output moves by more than the GPU test's allowance K u E"""
    return any(bool(((bad[n] - ref[n]).abs() > 2 * K * U * ref["E_" + n] + 1e-300).any()) for n in names)


@pytest.mark.parametrize("fault", P.FEAT_FAULTS)
def test_feature_composite_faults_exceed_every_bound(fault):
    for c in P.FEAT_CASES:
        if c["S"] == 1 and fault in ("T_i", "suffix_incl"):
            continue                                        # no density sample: d_sigma is identically zero
        if c["act"] == "none" and fault == "no_act_grad":
            continue                                        # act' is 1
        if c["sub"] == "w" and fault in ("no_act_grad", "drop_last_geo"):
            continue                                        # no g_fmap: d_rows is identically zero
        assert _exceeds(P.feat_reference(c), P.feat_reference(c, fault=fault), ("d_sigma", "d_rows")), (fault, c["id"])


def test_color_seeds_are_the_chosen_ones():
    for c in P.COLOR_CASES:
        assert P.COLOR_SEEDS[(c["R"], c["Lv"], c["bias"])] == P.choose_color_seed(c), c["id"]
        assert P.color_inputs(c)["unsure"].sum() <= P.UNSURE_CAP * c["R"]


COLOR_AUTOGRAD = [c for c in P.COLOR_CASES if c["R"] in (5, 257)]


@pytest.mark.parametrize("c", COLOR_AUTOGRAD, ids=[c["id"] for c in COLOR_AUTOGRAD])
def test_color_rows_backward_is_autograd(c):
    a, r = P.color_inputs(c), P.color_reference(c)
    Pm = {k: (v.clone().requires_grad_(True) if v is not None else None) for k, v in P.color_params(P.color_state_dict(c)).items()}
    fm = _t(a["fmap"]).double().requires_grad_(True)
    d = _t(a["rays"][:, a["col"]:a["col"] + 3]).double().requires_grad_(True)
    out = P.color_rows_autograd(Pm, fm, d, c["Lv"])
    assert float((out.detach() - r["color"]).abs().max()) < 1e-14
    (out * _t(a["g_color"]).double()).sum().backward()
    got = dict(d_map=fm.grad, d_dirs=d.grad, **{"d_" + k: v.grad for k, v in Pm.items() if v is not None})
    for k, g in got.items():
        assert float((g - r[k]).abs().max()) <= 1e-12 * max(1.0, float(r[k].abs().max())), k


def test_forward_order_reproduces_golden_G25():
    """activate the rows, composite, colour network per ray (voxnerf.py:223-239) on the golden's level inputs: l_feature, l_color to 1e-6"""
    g = load_golden("G25_pbe_composite_feature")
    gsz = W.pdrf_grid_size(V.AABB[0], V.AABB[1], 24 ** 3)
    sd = W.make_pdrf_state_dict(91, gsz, input_ch=95, hidden_dim=64, geo_feat_dim=15)
    R, S = g["l_z"].shape
    dirs = np.repeat(g["l_vd"].reshape(R, 1, 3), S, 1).reshape(-1, 3)
    with torch.no_grad():
        raw, geo = V.level_forward64(sd, g["l_pts"].reshape(-1, 3), dirs, g["l_fts"].reshape(R * S, -1), 10, 4)
        fmap = P.feat_composite_autograd(raw.reshape(R, S, 4)[..., 0], geo.reshape(R, S, -1), g["l_z"], _t(g["l_rd"]).double())[0]
        color = P.color_rows(P.color_params(sd), fmap, _t(g["l_vd"].reshape(R, 3)), 4)["color"]
    assert float(np.abs(fmap.numpy() - g["l_feature"]).max()) < 1e-6
    assert float(np.abs(color.numpy() - g["l_color"]).max()) < 1e-6


@pytest.mark.parametrize("fault", P.COLOR_FAULTS)
def test_color_rows_faults_exceed_every_bound(fault):
    names = ("color", "d_map", "d_w0", "d_w1", "d_w2")
    for c in P.COLOR_CASES:
        if c["Lv"] == 0 and fault == "sincos_swapped":
            continue                                        # no sin / cos columns
        assert _exceeds(P.color_reference(c), P.color_reference(c, fault=fault), names), (fault, c["id"])
