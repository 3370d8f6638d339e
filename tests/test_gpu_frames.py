"""8-bit pictures of frame stacks on the device (evdeblurnerf_amd.frames over evd_frame_range / evd_frame_map / evd_frame_colormap:
k_frame_range, k_frame_range_finish, k_frame_map, k_frame_colormap) against tests/frames_ref.py, the reference's statements executed by
NumPy.  Every comparison is exact uint8 equality: zero mismatching bytes, no tolerance.

Shapes (N, H, W): (1, 1, 1); (3, 37, 53) -- 1961 values per frame, 5883 floats per RGB frame: the slices of frames 1 and 2 start off
16-byte alignment and every vector path has a head and a tail; (5, 129, 131) -- 16899 values per frame: three workgroups per frame, the
finish launch folds more than one partial.  Data: uniform in [-0.2, 1.3] so that both clips act, the extreme (1.5) once in element 0 and
once in the very last element of the last frame, and in the frame that holds it a block of values k / 255 * 1.5, k = 0..255, where
float32 rounding decides the byte.

Constant frames: the stated deviation is about a slice whose DIVISOR is 0 (depth: maximum 0, i.e. disps == 1 before the inversion; error
map: prediction == ground truth; video: maximum == minimum); those give zeros.  A constant frame with a non-zero maximum is defined in
the reference (every value / max == 1) and gives 255 there and here."""
import numpy as np
import pytest
import torch

import frames_ref as R
from evdeblurnerf_amd import frames as F
from evdeblurnerf_amd import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (3, 37, 53), (5, 129, 131)]
EXT = np.float32(1.5)
# a random permutation per channel, not a smooth map: an index or channel-order error changes bytes
LUT = np.stack([np.random.RandomState(77 + c).permutation(256) for c in range(3)], -1).astype(np.uint8)


def T(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def N(x):
    return x.detach().cpu().numpy()


def same(got, want, what):
    got = N(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} bytes differ"


def stack(shape, where, seed):
    """values [N, H, W] (or any shape) whose maximum EXT sits in element 0 ('first') or in the last element of the last frame ('last'),
    with the k / 255 * EXT block in that frame"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.2, 1.3, shape).astype(np.float32)
    per = v[0].size
    f = v.reshape(shape[0], per)[0 if where == "first" else -1]
    k = np.arange(256, dtype=np.float32)[:max(0, min(256, per - 2))]
    f[1:1 + k.size] = k / np.float32(255) * EXT
    f[0 if where == "first" else -1] = EXT
    return v


_CASES = {}


def case(shape, where):
    """one seeded stack per (shape, where), computed once and shared read-only"""
    key = (shape, where)
    if key not in _CASES:
        _CASES[key] = stack(shape, where, 4100 + 7 * shape[1] + (where == "last"))
    return _CASES[key]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_images(shape, where):
    v = case(shape, where)
    for invert in (False, True):
        d = np.float32(1.) - v if invert else v         # the VALUE 1 - d then carries the extreme and, to a rounding, the block
        dt = T(d)
        for scope in ("all", "frame"):
            for lut in (None, LUT):
                got = F.depth_images(dt, invert=invert, scope=scope, colormap=None if lut is None else T(lut))
                same(got, R.depth_images(d, invert, scope, lut), f"depth_images {shape} {where} invert={invert} {scope} lut={lut is not None}")
    g = R.depth_images(v, False, "all")
    assert g.max() == 255 and (shape == (1, 1, 1) or (g.min() == 0 and (v < 0).any() and len(np.unique(g)) > 250))      # both clips act


@pytest.mark.parametrize("shape", SHAPES)
def test_depth_images_layouts(shape):
    """other dtypes are converted, non-contiguous input is made contiguous, the table may be a NumPy array; two runs give the same bytes"""
    v = case(shape, "last")
    want = R.depth_images(v, True, "frame", LUT)
    same(F.depth_images(T(v.astype(np.float64)), scope="frame", colormap=LUT), want, "float64 input")
    wide = T(np.concatenate([v, v], -1))
    same(F.depth_images(wide[..., :shape[2]], scope="frame", colormap=LUT), want, "non-contiguous input")
    a, b = F.depth_images(T(v), scope="frame", colormap=LUT), F.depth_images(T(v), scope="frame", colormap=LUT)
    assert torch.equal(a, b)
    grey = F.depth_images(T(v), scope="frame")
    same(F.apply_colormap(255 - grey, LUT), want, "apply_colormap(255 - grey)")
    same(F.apply_colormap(grey.reshape(-1)[1:], T(LUT)), LUT[N(grey).reshape(-1)[1:]], "apply_colormap on an unaligned view")


def test_constant_frames():
    """a slice whose divisor is 0 is grey level 0 (through a table: its row 255), by itself and among others"""
    ones = np.ones((1, 37, 53), np.float32)
    for scope in ("frame", "all"):
        assert not N(F.depth_images(T(ones), invert=True, scope=scope)).any()
        assert not N(F.depth_images(T(0 * ones), invert=False, scope=scope)).any()
    assert (N(F.depth_images(T(ones), invert=True, scope="frame", colormap=LUT)) == LUT[255]).all()
    same(F.depth_images(T(0.25 * ones), invert=False, scope="frame"), np.full(ones.shape, 255, np.uint8), "a non-zero constant frame")
    v = case((3, 37, 53), "last").copy()
    v[1] = 1.0                                           # 1 - 1 = 0 throughout frame 1
    got = F.depth_images(T(v), invert=True, scope="frame")
    assert not N(got)[1].any()
    same(got, R.depth_images(v, True, "frame"), "a constant frame among others")
    same(F.depth_images(T(v), invert=True, scope="all", colormap=LUT), R.depth_images(v, True, "all", LUT), "the same stack, one maximum")
    rgb = np.random.RandomState(5).uniform(-0.2, 1.3, (3, 37, 53, 3)).astype(np.float32)
    gt = np.random.RandomState(6).uniform(-0.2, 1.3, rgb.shape).astype(np.float32)
    gt[1] = rgb[1]
    e = F.error_maps(T(rgb), T(gt))
    assert not N(e)[1].any()
    same(e, R.error_maps(rgb, gt), "error map with an exact frame")
    assert not N(F.video_frames(T(np.full((2, 5, 7, 3), 0.7, np.float32)))).any()


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_one_nan_pixel(shape):
    """a NaN pixel is 0 and every other byte is what np.nanmax / np.nanmin give"""
    v = case(shape, "first").copy()
    pos = (shape[0] - 1, shape[1] // 2, shape[2] - 1)
    v[pos] = np.nan
    for scope in ("all", "frame"):
        for invert in (False, True):
            got = F.depth_images(T(v), invert=invert, scope=scope)
            assert N(got)[pos] == 0
            same(got, R.depth_images(v, invert, scope), f"NaN {scope} invert={invert}")
    same(F.depth_images(T(v), invert=False, scope="frame", colormap=LUT), R.depth_images(v, False, "frame", LUT), "NaN through the table")
    rgb, gt = rgb_pair(shape, "first")
    rgb = rgb.copy()
    rgb[pos + (1,)] = np.nan
    got = F.error_maps(T(rgb), T(gt))
    assert N(got)[pos] == 0
    same(got, R.error_maps(rgb, gt), "NaN in an error map")
    got = F.video_frames(T(rgb))
    assert N(got)[pos + (1,)] == 0
    same(got, R.video_frames(rgb), "NaN in the video frames")


def rgb_pair(shape, where):
    """prediction and ground truth [N, H, W, 3] whose per-pixel error has its maximum in pixel 0 / the last pixel of the last frame and, in
    that frame, a block of errors near k / 255 of it"""
    key = ("rgb",) + (shape, where)
    if key not in _CASES:
        n, h, w = shape
        rs = np.random.RandomState(4300 + 7 * h + (where == "last"))
        gt = rs.uniform(-0.2, 1.3, (n, h, w, 3)).astype(np.float32)
        rgb = (gt + rs.uniform(-0.5, 0.5, gt.shape)).astype(np.float32)           # errors up to 0.25
        f_rgb, f_gt = (a.reshape(n, h * w, 3)[0 if where == "first" else -1] for a in (rgb, gt))
        k = np.arange(256, dtype=np.float32)[:max(0, min(256, h * w - 2))]
        f_rgb[1:1 + k.size] = f_gt[1:1 + k.size] + np.sqrt(k / np.float32(255))[:, None]      # mean squared error ~ k / 255
        f_rgb[0 if where == "first" else -1] = f_gt[0 if where == "first" else -1] + np.float32(1.0)
        _CASES[key] = (rgb, gt)
    return _CASES[key]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", SHAPES)
def test_error_maps(shape, where):
    rgb, gt = rgb_pair(shape, where)
    for lut in (None, LUT):
        same(F.error_maps(T(rgb), T(gt), colormap=lut), R.error_maps(rgb, gt, lut), f"error_maps {shape} {where} lut={lut is not None}")
    if shape != (1, 1, 1):
        # sources whose slices share no 16-byte phase go element by element: the same bytes
        flat = torch.empty(rgb.size + 1, dtype=torch.float32, device=DEV)
        flat[1:] = T(rgb).reshape(-1)
        same(F.error_maps(flat[1:].view(rgb.shape), T(gt)), R.error_maps(rgb, gt), "error_maps, prediction one float off alignment")


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", SHAPES)
def test_video_frames(shape, where):
    n, h, w = shape
    x = stack((n, h, w, 3), where, 4500 + 7 * h + (where == "last"))
    lo = np.float32(-0.5)
    f = x.reshape(n, -1)[0 if where == "first" else -1]
    k = np.arange(256, dtype=np.float32)[:max(0, min(256, f.size - 2))]
    f[1:1 + k.size] = lo + k / np.float32(255) * (EXT - lo)
    f[1 if where == "first" else -2] = lo                # the minimum next to the maximum
    same(F.video_frames(T(x)), R.video_frames(x), f"video_frames {shape} {where}")
    off = torch.empty(x.size + 3, dtype=torch.float32, device=DEV)
    off[3:] = T(x).reshape(-1)
    same(F.video_frames(off[3:].view(x.shape)), R.video_frames(x), "video_frames, three floats off alignment")


# ------------------------------------------------------------------------------------------------ the two passes
@pytest.fixture(scope="module")
def tiny():
    """a tiny c2f model (both PDRF levels on 16^3 / 24^3-voxel grids), 2 poses at 24 x 24, 16 + 16 samples, perturb 0"""
    from evdeblurnerf_amd.renderer import NeRFAll
    from evdeblurnerf_amd.tonemapping import TonemappingTransform
    cv, fv = 16 ** 3, 24 ** 3
    model = NeRFAll(W.blurfactory_args(16, cv, fv), W.make_blurfactory_state_dict(31, cv, fv, sigma_gain=3.0), precision="f16x3").eval()
    crf = TonemappingTransform("gamma", "gamma")
    H = Wd = 24
    kw = dict(ndc=True, near=0., far=1., use_viewdirs=True, N_samples=16, N_importance=16, perturb=0., raw_noise_std=0.)
    poses = [W.synthetic_pose(70 + i) for i in range(2)]
    gts = W.synthetic_frame_pairs(9, 2, H, Wd)[1]
    return model, crf, H, Wd, W.synthetic_camera(H, Wd, 30.0), poses, gts, kw


def test_test_set_pass(tiny):
    from evdeblurnerf_amd import metrics as M
    model, crf, H, Wd, K, poses, gts, kw = tiny
    for lut in (None, LUT):
        out = F.test_set_pass(model, crf, H, Wd, K, 1 << 20, poses, T(gts), kw, colormap=lut)
        rgbs, disps = out["rgbs"], out["disps"]
        assert rgbs.is_cuda and rgbs.shape == (2, H, Wd, 3) and disps.shape == (2, H, Wd) and rgbs.dtype == torch.float32
        assert float(rgbs.std()) > 1e-3                                                # a picture, not a constant
        same(out["rgb8"], R.to8b(N(rgbs)), "test_set_pass rgb8")
        same(out["gt8"], R.to8b(gts), "test_set_pass gt8")
        same(out["depth8"], R.depth_images(N(disps), True, "all", lut), "test_set_pass depth8")
        same(out["err8"], R.error_maps(N(rgbs), gts, lut), "test_set_pass err8")
        assert set(out["metrics"]) == {"mse", "psnr", "ssim"}
        for m, val in out["metrics"].items():
            assert isinstance(val, float) and val == M.compute_img_metric(rgbs, T(gts), m), m
    assert set(F.test_set_pass(model, crf, H, Wd, K, 1 << 20, poses, T(gts), kw, metrics=("psnr",))["metrics"]) == {"psnr"}


def test_video_pass(tiny):
    model, crf, H, Wd, K, poses, gts, kw = tiny
    out = F.video_pass(model, crf, H, Wd, K, 1 << 20, poses, kw)
    rgbs, disps = out["rgbs"], out["disps"]
    assert rgbs.is_cuda and rgbs.shape == (2, H, Wd, 3) and disps.shape == (2, H, Wd)
    same(out["rgb8"], R.video_frames(N(rgbs)), "video_pass rgb8")
    same(out["disp8"], R.depth_images(N(disps), False, "all"), "video_pass disp8")
    assert N(out["rgb8"]).min() == 0 and N(out["rgb8"]).max() == 255
