"""The TV regulariser of a PDRF level on the GPU, alone: evd_voxel_tv_loss (k_tv_level / k_tv_finish) and evd_voxel_tv_loss_bwd
(k_tv_bwd_level) through the raw library entries with a VoxelGridGrads built by hand, against the float64 reference tests/tv_ref.py, and
once through VoxelNeRFBase.tv_loss_train.

Levels (grid sizes through W.pdrf_grid_size; tests/test_tv_ref.py checks the boxes on the CPU):
  [27, 27, 18]    the box of test_triplane_sample_and_tv_backward_match_torch_autograd: the baseline
  [65, 2, 3]      axes of size 2 (a row that is both the first and the last but one); line 2 has 65 entries, one past tv_by's cap of 64
  [2, 66, 3]      the same with the axes swapped: plane 0 is 66 x 2
  [1100, 70, 3]   plane 0 is 70 x 1100 x 64: 17600 vec4 per row > 64 * 256 (tv_bx's cap), 70 rows > 64 (tv_by's cap), 1.23 M vec4 > 4096 * 256
                  (the backward's cap) -- all three strided loops run
each with app_n_comp (64, 16, 16), as shipped, and (8, 32, 16), whose counts all differ (a wrong tensor-to-job mapping shows).  The grids
are random normals.

Bounds, in units of u = 2^-24, from counting roundings (not from what the kernels give):
  value      |got - ref| <= 8 u ref: a vec4's sum of squared float32 differences is a sum of non-negative terms with at most 5 roundings
             along any path (difference, square, three additions), accumulated in double, rounded once to float32, with slack to 8.
  gradient   |got - ref| <= 16 u A elementwise, A = tv_ref's sum of the absolute terms: per term 1 (difference) + at most 4 (kh / kw: the
             float32 weight constant, d_loss x weight, the count product, the division) + 1 (product) + at most 4 (the running sum of four
             terms, counted against the whole of A) + 1 (the add into the gradient) = 11, with slack to 16.
  add        into a pre-filled g0: the bound above + u |g0 + tv_grad| (the one add into the buffer rounds at the size of the result);
             twice: g0 + 2 tv_grad within twice that, 32 u A + 2 u |g0 + 2 tv_grad| (the first add rounds at |g0 + tv_grad| <=
             |g0 + 2 tv_grad| + A, and the count above leaves more than that one u A unused).
The measured worst error / bound of each family is printed by the test (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tv_ref
from evdeblurnerf_amd import weights as W

gpu = pytest.mark.gpu
U = 2.0 ** -24
BASE_AABB = ([-1.5, -1.5, -1.0], [1.5, 1.5, 1.0])
LEVELS = [(27, 27, 18), (65, 2, 3), (2, 66, 3), (1100, 70, 3)]
N_COMP = [(64, 16, 16), (8, 32, 16)]
CASES = [(g, c) for g in LEVELS for c in N_COMP]
IDS = ["x".join(map(str, g)) + "-" + "_".join(map(str, c)) for g, c in CASES]


def level_box(grid):
    """(aabb_min, aabb_max, n_voxels) whose grid size under the reference's rule (voxnerf.py:88-93) is `grid`"""
    if tuple(grid) == (27, 27, 18):
        return BASE_AABB[0], BASE_AABB[1], 24 ** 3
    ext = [(g + 0.5) / 100.0 for g in grid]
    return [-e / 2 for e in ext], [e / 2 for e in ext], int(round(float(np.prod([g + 0.5 for g in grid]))))


class Level:
    def __init__(self, grid, n_comp):
        from evdeblurnerf_amd.voxnerf import VoxelNeRFRayFeatures
        lo, hi, n_vox = level_box(grid)
        assert W.pdrf_grid_size(lo, hi, n_vox) == list(grid)
        sd = W.make_pdrf_state_dict(71, list(grid), input_ch=95, hidden_dim=64, geo_feat_dim=15, app_n_comp=n_comp, grid_scale=1.0)
        self.net = VoxelNeRFRayFeatures(sd, "", (lo, hi), num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3, input_ch=95,
                                       app_dim=32, app_n_comp=n_comp, n_voxels=n_vox)
        assert self.net.gridSize == list(grid)
        self.planes, self.lines = tv_ref.from_state_dict(sd)
        self.shapes = [tuple(t.shape) for t in self.planes] + [(t.shape[0], t.shape[2]) for t in self.lines]     # device layouts
        self.value = float(tv_ref.value(self.planes, self.lines))
        g, a = tv_ref.level_grad(self.planes, self.lines, 1.0)
        # the reference weights are the doubles 1e-2 / 1e-3, the kernel's the float32 constants: counted among kh / kw's roundings
        self.grad = [t.reshape(s) for t, s in zip(g, self.shapes)]
        self.A = [t.reshape(s) for t, s in zip(a, self.shapes)]
        self.edge = [tv_ref.edge_mask(t).reshape(s) for t, s in zip(self.planes + self.lines, self.shapes)]

    def tv(self):
        from evdeblurnerf_amd import _lib as L
        out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
        L.check(L.lib().evd_voxel_tv_loss(self.net._h, L.ptr(out), L.stream_ptr()), "evd_voxel_tv_loss")
        return float(out.cpu()[0])

    def bwd(self, d_loss, bufs):
        """evd_voxel_tv_loss_bwd with bufs[i] (a device tensor or None = a null pointer) for planes 0..2, lines 0..2"""
        from evdeblurnerf_amd import _lib as L
        gs = L.VoxelGridGrads()
        for i in range(3):
            gs.plane[i] = bufs[i].data_ptr() if bufs[i] is not None else None
            gs.line[i] = bufs[3 + i].data_ptr() if bufs[3 + i] is not None else None
        gs.basis = None
        d = torch.tensor([d_loss], dtype=torch.float32, device="cuda")
        L.check(L.lib().evd_voxel_tv_loss_bwd(self.net._h, L.ptr(d), C.byref(gs), L.stream_ptr()), "evd_voxel_tv_loss_bwd")
        torch.cuda.synchronize()

    def zeros(self):
        return [torch.zeros(s, dtype=torch.float32, device="cuda") for s in self.shapes]


_levels = {}


def get_level(key):
    if key not in _levels:
        _levels[key] = Level(*key)
    return _levels[key]


@pytest.fixture
def level(request):
    return get_level(request.param)


def worst(err, bound):
    """max over the elements of err / bound (0 / 0 counts as 0)"""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def check_grads(lv, got, d_loss, g0=None, times=1, what=""):
    """got[i] against g0 + times * d_loss * grad within times * (16 u |d_loss| A [+ u |result|]), per tensor and on the edge set"""
    d = float(np.float32(d_loss))
    ratios = []
    for i, t in enumerate(got):
        ref = times * d * lv.grad[i]
        bound = times * 16 * U * abs(d) * lv.A[i]
        if g0 is not None:
            ref = ref + g0[i]
            bound = bound + times * U * ref.abs()
        err = (t.cpu().double() - ref).abs()
        name = ("plane", "line")[i // 3] + str(i % 3)
        r_all, r_edge = worst(err, bound), worst(err[lv.edge[i]], bound[lv.edge[i]])
        ratios.append(r_all)
        assert r_all <= 1.0, f"{what} {name}: error {r_all:.3g} x the bound"
        assert r_edge <= 1.0, f"{what} {name}, edge rows and columns: error {r_edge:.3g} x the bound"
    print(f"tv {what}: worst error / bound = {max(ratios):.3f}")


@gpu
@pytest.mark.parametrize("level", CASES, ids=IDS, indirect=True)
def test_value(level):
    got = level.tv()
    print(f"tv value: |got - ref| / (8 u ref) = {abs(got - level.value) / (8 * U * level.value):.3f}")
    assert abs(got - level.value) <= 8 * U * level.value


@gpu
@pytest.mark.parametrize("d_loss", [1.0, 5e-2, -3.0])
@pytest.mark.parametrize("level", CASES, ids=IDS, indirect=True)
def test_gradient_into_zeroed_buffers_scales_with_the_upstream_scalar(level, d_loss):
    bufs = level.zeros()
    level.bwd(d_loss, bufs)
    check_grads(level, bufs, d_loss, what=f"zeroed d_loss={d_loss:g}")


@gpu
@pytest.mark.parametrize("level", CASES, ids=IDS, indirect=True)
def test_gradient_adds_into_a_prefilled_buffer(level):
    gen = torch.Generator().manual_seed(9)
    scale = [float(g.abs().mean()) for g in level.grad]
    g0 = [(torch.randn(s, generator=gen, dtype=torch.float64) * 3 * sc).float().double() for s, sc in zip(level.shapes, scale)]
    bufs = [t.float().cuda() for t in g0]
    level.bwd(1.0, bufs)
    check_grads(level, bufs, 1.0, g0=g0, what="pre-filled")
    level.bwd(1.0, bufs)
    check_grads(level, bufs, 1.0, g0=g0, times=2, what="pre-filled, twice")


@gpu
@pytest.mark.parametrize("wanted", [(4,), (1, 2, 3, 4, 5)], ids=["only-line1", "all-but-plane0"])
@pytest.mark.parametrize("level", CASES, ids=IDS, indirect=True)
def test_null_gradient_pointers_are_skipped(level, wanted):
    sentinel = -1.2345678e9
    bufs = level.zeros()
    spare = [torch.full(s, sentinel, dtype=torch.float32, device="cuda") for s in level.shapes]
    before = [t.clone() for t in spare]
    level.bwd(1.0, [bufs[i] if i in wanted else None for i in range(6)])
    for i in range(6):
        if i in wanted:
            err = (bufs[i].cpu().double() - level.grad[i]).abs()
            assert worst(err, 16 * U * level.A[i]) <= 1.0, f"tensor {i}"
        else:
            assert not bool(bufs[i].any()), f"tensor {i} was written without a pointer to it"
        assert torch.equal(spare[i].view(torch.int32), before[i].view(torch.int32)), f"a buffer the call never saw changed ({i})"


@gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_autograd_path_equals_the_raw_entry(in_place):
    lv = get_level(((27, 27, 18), (64, 16, 16)))
    raw = lv.zeros()
    lv.bwd(1.0, raw)
    net = lv.net
    grids = net.grid_params()
    net._grads_in_place = in_place
    try:
        tv = net.tv_loss_train(grids)
        assert float(tv.detach()) == lv.tv()
        tv.backward()
    finally:
        del net._grads_in_place
    for i in range(6):
        assert torch.equal(grids[i].grad, raw[i]), f"tensor {i}"
    assert grids[6].grad is None or not bool(grids[6].grad.any()), "the basis receives nothing from TV"
