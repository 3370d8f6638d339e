"""Pins the float64 TV reference of tests/test_gpu_tv.py (tests/tv_ref.py) before any kernel is held to it: its value to the torch
restatement of TVLoss and to the CPU oracle, its closed-form gradient to torch float64 autograd of the value, and the bound scale A to its
definition.  Also checks, without a GPU, that the boxes and voxel counts of tests/test_gpu_tv.py give the grid sizes they are meant to.
CPU only."""
import numpy as np
import pytest
import torch

import tv_ref
from evdeblurnerf_amd import weights as W
from oracle import oracle as O
from torch_restatement import torch_tv

GRIDS = [[27, 27, 18], [65, 2, 3], [2, 66, 3], [5, 4, 3]]
N_COMP = [(64, 16, 16), (8, 32, 16)]


def _level(seed, grid, n_comp):
    return W.make_pdrf_state_dict(seed, grid, input_ch=95, hidden_dim=64, geo_feat_dim=15, app_n_comp=n_comp, grid_scale=1.0)


@pytest.mark.parametrize("n_comp", N_COMP)
@pytest.mark.parametrize("grid", GRIDS)
def test_value_matches_the_torch_restatement_and_the_oracle(grid, n_comp):
    sd = _level(3, grid, n_comp)
    planes, lines = tv_ref.from_state_dict(sd)
    got = float(tv_ref.value(planes, lines))
    ref = sum(float(torch_tv(torch.as_tensor(sd[f"app_plane.{i}"]).double())) * 1e-2
              + float(torch_tv(torch.as_tensor(sd[f"app_line.{i}"]).double())) * 1e-3 for i in range(3))
    assert abs(got - ref) <= 1e-13 * ref                   # the same float64 sums in another layout
    orc = sum(O.tv_loss(sd[f"app_plane.{i}"]) * 1e-2 + O.tv_loss(sd[f"app_line.{i}"]) * 1e-3 for i in range(3))
    assert abs(got - orc) <= 1e-5 * got                    # the oracle restates TVLoss in float32 (tests/test_gpu_parity.py's bound)


@pytest.mark.parametrize("upstream", [1.0, 5e-2, -3.0])
@pytest.mark.parametrize("n_comp", N_COMP)
@pytest.mark.parametrize("grid", GRIDS)
def test_closed_form_gradient_matches_autograd(grid, n_comp, upstream):
    planes, lines = tv_ref.from_state_dict(_level(4, grid, n_comp))
    leaves = [t.clone().requires_grad_(True) for t in planes + lines]
    (upstream * tv_ref.value(leaves[:3], leaves[3:])).backward()
    grads, A = tv_ref.level_grad(planes, lines, upstream)
    for i, (g, a, t) in enumerate(zip(grads, A, leaves)):
        assert g.shape == t.shape and a.shape == t.shape
        # both are float64 evaluations of the same at most four terms: a few 2^-53 of the sum of their absolute values
        assert bool(((g - t.grad).abs() <= 1e-14 * a).all()), f"tensor {i}"
        assert bool((g.abs() <= a * (1 + 1e-14)).all())


def test_bound_scale_is_the_sum_of_the_absolute_terms():
    rs = np.random.RandomState(5)
    x = torch.tensor(rs.standard_normal((4, 3, 8)))
    H, W_, C = x.shape
    scale = -0.7
    kh, kw = 4 * scale / (C * (H - 1) * W_), 4 * scale / (C * H * (W_ - 1))
    g, a = tv_ref.grad(x, scale)
    for h in range(H):
        for w in range(W_):
            c = x[h, w]
            terms = []
            if h > 0:
                terms.append(kh * (c - x[h - 1, w]))
            if h + 1 < H:
                terms.append(-kh * (x[h + 1, w] - c))
            if w > 0:
                terms.append(kw * (c - x[h, w - 1]))
            if w + 1 < W_:
                terms.append(-kw * (x[h, w + 1] - c))
            assert torch.allclose(g[h, w], sum(terms), rtol=0, atol=1e-15)
            assert torch.allclose(a[h, w], sum(t.abs() for t in terms), rtol=0, atol=1e-15)
    line = torch.tensor(rs.standard_normal((5, 1, 4)))
    gl, al = tv_ref.grad(line, 1.0)
    ref = torch.zeros_like(line)
    d = line[1:] - line[:-1]
    ref[1:] += d
    ref[:-1] -= d
    assert torch.allclose(gl, ref * 4 / (4 * 4 * 1), rtol=0, atol=1e-15)   # a line has no width term
    with pytest.raises(ValueError):
        tv_ref.reg(torch.zeros((1, 3, 4), dtype=torch.float64))


def test_edge_mask():
    m = tv_ref.edge_mask(torch.zeros((5, 4, 2)))
    assert int(m.sum()) == (5 * 4 - 3 * 2) * 2
    assert bool(tv_ref.edge_mask(torch.zeros((6, 1, 2))).all())


def test_gpu_test_boxes_give_their_grid_sizes():
    """the (box, voxel count) pairs of tests/test_gpu_tv.py, through the reference's grid-size rule"""
    from test_gpu_tv import LEVELS, level_box
    for grid in LEVELS:
        lo, hi, n_vox = level_box(grid)
        assert W.pdrf_grid_size(lo, hi, n_vox) == list(grid), grid
