"""Pins the float64 tri-plane reference of tests/test_gpu_triplane.py (tests/triplane_ref.py) before any kernel is held to it:
to the golden features the real reference computed (G8), to the CPU oracle on the edge point sets, and its explicit backward to
torch autograd through F.grid_sample.  CPU only."""
import numpy as np
import torch

from conftest import load_golden
from evdeblurnerf_amd import weights as W
from oracle import oracle as O
from torch_restatement import torch_appfeature
from triplane_ref import edge_points, index_points, src_indices, to_channel_last, triplane

AABB = ([-1.5, -1.5, -1.0], [1.5, 1.5, 1.0])
U32 = 2.0 ** -24


def _sd(seed, nvox, n_comp=(64, 16, 16), fine=False):
    g = W.pdrf_grid_size(AABB[0], AABB[1], nvox)
    net = dict(input_ch=127, hidden_dim=256, geo_feat_dim=128) if fine else dict(input_ch=95, hidden_dim=64, geo_feat_dim=15)
    sd = W.make_pdrf_state_dict(seed, g, app_n_comp=n_comp, **net)
    return sd, g


def test_reference_reproduces_the_golden_appfeature():
    """G8: features the reference's VoxelNeRFBase.sample produced (float32 torch) at seeds 21 / 22; float64 here, 2e-6 apart at most"""
    g = load_golden("G8_appfeature")
    pts = g["pts"].reshape(-1, 3)
    for seed, nvox, key in ((21, 24 ** 3, "ft_coarse"), (22, 48 ** 3, "ft_fine")):
        sd, grid = _sd(seed, nvox, fine=key == "ft_fine")
        assert list(grid) == list(g["grid_coarse" if key == "ft_coarse" else "grid_fine"])
        pl, li, ba = to_channel_last(sd)
        src, _ = src_indices(pts, AABB, grid)
        r = triplane([torch.tensor(p) for p in pl], [torch.tensor(l) for l in li], torch.tensor(ba), src)
        ref = g[key].reshape(-1, 32).astype(np.float64)
        err = np.abs(r["out"].numpy() - ref)
        assert err.max() < 2e-6, (key, err.max())
        # the golden is float32 arithmetic: within a float32-grade multiple of the magnitude, element by element
        assert (err <= 120 * U32 * r["out_m"].numpy() + 1e-30).all(), key


def test_edge_points_hit_the_wanted_float32_indices():
    """index_points steps the float32 pipeline until the source index IS the wanted value: both faces of every axis, and the exact
    integers edge_points keeps are exactly those"""
    rs = np.random.RandomState(3)
    for nvox in (24 ** 3, 134217984):
        grid = W.pdrf_grid_size(AABB[0], AABB[1], nvox)
        want = np.full((6, 3), np.nan)
        for a in range(3):
            want[2 * a, a], want[2 * a + 1, a] = 0.0, grid[a] - 1
        src, _ = src_indices(index_points(AABB, grid, want, rs), AABB, grid)
        ok = ~np.isnan(want)
        assert (src[ok] == want[ok]).all(), src[ok]
        src, _ = src_indices(edge_points(AABB, grid, rs), AABB, grid)
        for a in range(3):
            ints = src[(src[:, a] == np.floor(src[:, a])) & (src[:, a] > 0) & (src[:, a] < grid[a] - 1), a]
            assert len(set(ints.tolist())) >= 1, (nvox, a)


def test_reference_matches_the_oracle_on_edge_points():
    """the CPU oracle (float32 C, the ATen CPU kernel's form) on box faces, exact integers, ulp neighbours and far points, at the
    shipped n_comp and at one that is not a multiple of 8"""
    rs = np.random.RandomState(5)
    for n_comp, nvox in (((64, 16, 16), 24 ** 3), ((48, 12, 12), 20 ** 3)):
        sd, grid = _sd(9, nvox, n_comp)
        pts = edge_points(AABB, grid, rs)
        v = O.Voxel(sd, "", grid, AABB[0] + AABB[1], input_ch=95, n_comp=n_comp)
        got = O.appfeature(v, pts).astype(np.float64)
        pl, li, ba = to_channel_last(sd)
        src, _ = src_indices(pts, AABB, grid)
        r = triplane([torch.tensor(p) for p in pl], [torch.tensor(l) for l in li], torch.tensor(ba), src)
        ct = sum(n_comp)
        err = np.abs(got - r["out"].numpy())
        bound = (ct + 16) * U32 * r["out_m"].numpy()
        assert (err <= bound).all(), (n_comp, float((err / np.maximum(bound, 1e-300)).max()))
        # far and outside points: exactly zero in both
        outside = np.any((pts < np.array(AABB[0]) - 0.2) | (pts > np.array(AABB[1]) + 0.2), 1)
        assert outside.sum() >= 9 and (got[outside] == 0).all() and (r["out"].numpy()[outside] == 0).all()


def test_reference_backward_matches_autograd_through_grid_sample():
    """the explicit float64 backward (grid, line and basis gradients; d pts through the interpolation weights with ATen's one-sided
    convention) against torch autograd on F.grid_sample in float64, at random in-box and outside points"""
    sd, grid = _sd(13, 16 ** 3, (16, 8, 8))
    rs = np.random.RandomState(17)
    pts = (rs.uniform(-1.7, 1.7, (300, 3)) * np.array([1.0, 1.0, 0.7])).astype(np.float32)
    d_out = rs.normal(size=(300, 32))
    pl, li, ba = to_channel_last(sd)
    src, k = src_indices(pts, AABB, grid)
    r = triplane([torch.tensor(p) for p in pl], [torch.tensor(l) for l in li], torch.tensor(ba), src, kpts=k, d_out=d_out)
    # the autograd side: F.grid_sample on normalised coordinates made from the same float32 source indices (float64 round trip,
    # ~1e-15 cells), d pts = d index x k by the chain rule
    s64 = torch.tensor(src, dtype=torch.float64, requires_grad=True)
    gsz = torch.tensor([float(g - 1) for g in grid], dtype=torch.float64)
    xyz = s64 / gsz * 2 - 1
    planes = [torch.tensor(np.asarray(sd[f"app_plane.{i}"]), dtype=torch.float64, requires_grad=True) for i in range(3)]
    lines = [torch.tensor(np.asarray(sd[f"app_line.{i}"]), dtype=torch.float64, requires_grad=True) for i in range(3)]
    basis = torch.tensor(np.asarray(sd["basis_mat.weight"]), dtype=torch.float64, requires_grad=True)
    out = torch_appfeature(planes, lines, basis, (xyz + 1) / 2 * torch.tensor(AABB[1], dtype=torch.float64).sub(torch.tensor(AABB[0], dtype=torch.float64))
                           + torch.tensor(AABB[0], dtype=torch.float64), AABB)
    (out * torch.tensor(d_out)).sum().backward()
    d_src = s64.grad
    close = lambda a, b, m: float(((a - b).abs() / (m + 1e-300)).max())
    assert close(r["out"], out.detach(), r["out_m"]) < 1e-6
    for i in range(3):
        assert close(r["d_plane"][i], planes[i].grad[0].permute(1, 2, 0), r["d_plane_m"][i]) < 1e-6, i
        assert close(r["d_line"][i], lines[i].grad[0, :, :, 0].t(), r["d_line_m"][i]) < 1e-6, i
    assert close(r["d_basis"], basis.grad, r["d_basis_m"]) < 1e-6
    assert close(r["d_pts"], d_src * torch.tensor(k), r["d_pts_m"]) < 1e-6


def test_reference_d_pts_at_an_exact_face_takes_the_outside_tap_as_zero():
    """ATen's convention at an exact integer index: the taps are floor(i) and floor(i) + 1 and the derivative is their difference,
    so at index size - 1 the outside tap enters as a zero value: d pv / d ix = -v(size - 1)"""
    sd, grid = _sd(13, 16 ** 3, (16, 8, 8))
    pl, li, ba = to_channel_last(sd)
    rs = np.random.RandomState(1)
    src = np.stack([np.array([grid[0] - 1, 0, 3], np.float32), rs.uniform(0, grid[1] - 1, 3), rs.uniform(0, grid[2] - 1, 3)], 1).astype(np.float32)
    k = np.array([0.7, 1.0, 1.0])
    r = triplane([torch.tensor(p) for p in pl], [torch.tensor(l) for l in li], torch.tensor(ba), src, kpts=k, d_out=np.ones((3, 32)))
    # the same derivative by a one-sided float64 difference to the right, taken on the float64 interpolation itself
    h = 2.0 ** -20
    s2 = src.astype(np.float64).copy()
    s2[:, 0] += h
    r2 = triplane([torch.tensor(p) for p in pl], [torch.tensor(l) for l in li], torch.tensor(ba), s2)
    fd = (r2["out"].sum(1) - r["out"].sum(1)) / h * k[0]
    assert torch.allclose(r["d_pts"][:, 0], fd, rtol=1e-4, atol=1e-9), (r["d_pts"][:, 0], fd)
