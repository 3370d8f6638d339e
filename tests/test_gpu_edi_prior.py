"""The EDI prior table on the device (evd_edi_prior: k_edi_windows, k_edi_prior_splat, k_edi_prior_deblur) against the float64 restatement
tests/edi_prior_ref.py, which tests/test_edi_prior_ref.py pins to the reference's own result (golden G36): every element within 2 u E,
the window indices exactly; bit-reproducible whatever the chunking; through EventTables and into ImageBatcher."""
import numpy as np
import pytest
import torch

import edi_prior_ref as R
from test_edi_prior_ref import g36_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def N(x):
    return x.detach().cpu().numpy()


def run(d, **kw):
    from evdeblurnerf_amd.edi import compute_edi_prior
    return compute_edi_prior(T(d["events"]), T(d["id_to_coords"]), d["tms_start"], d["tms_end"], T(d["images"]), d["steps"], d["cpos"], d["cneg"], **kw)


def ref_of(d):
    return R.edi_prior_ref(d["events"], d["id_to_coords"], d["tms_start"], d["tms_end"], d["images"], d["steps"], d["cpos"], d["cneg"])


def check(got, r, label):
    got = N(got)
    assert got.dtype == np.float32 and got.shape == r["prior"].shape
    worst = R.worst_ratio(got, r["prior"], r["E"])
    print(f"{label}: worst err / (u E) = {worst:.3f} over {got.size} elements")
    assert np.array_equal(np.isfinite(got), np.isfinite(r["prior"])) and worst <= R.K, (label, worst)
    return worst


def stream(seed, h, w, n_ev, n_img, steps=9, flt=True, cpos=0.2, cneg=0.25, exposure=10_000, gap=2_000, hot=0.05):
    """a seeded event table in the form EventTables keeps it: float32-valued coordinates as float64, integer microseconds, +-1"""
    rs = np.random.RandomState(seed)
    n_coords = h * w
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cx, cy = gx.reshape(-1), gy.reshape(-1)
    if flt:                                          # a smooth rectification, shifted right / down: taps fall off those two edges, none below 0
        cx, cy = cx + 0.31 * np.sin(0.04 * cy) + 0.45, cy + 0.27 * np.cos(0.03 * cx) + 0.35
    i2c = np.stack([cx, cy], -1).astype(np.float32).astype(np.float64)
    ids = rs.randint(0, n_coords, n_ev)
    pile = rs.rand(n_ev) < hot                       # a few pixels take many events per window
    ids[pile] = rs.randint(0, n_coords, 16)[rs.randint(0, 16, int(pile.sum()))]
    start = 500_000.0 + (exposure + gap) * np.arange(n_img)
    end = start + exposure
    t = np.sort(rs.randint(int(start[0]) - gap, int(end[-1]) + gap, n_ev)).astype(np.float64)
    p = np.where(rs.rand(n_ev) < 0.5, 1.0, -1.0)
    images = rs.uniform(0.02, 1.0, (n_img, h, w, 3)).astype(np.float32)
    return {"events": np.stack([ids.astype(np.float64), t, p, np.zeros(n_ev)], -1), "id_to_coords": i2c, "tms_start": start, "tms_end": end,
            "images": images, "steps": steps, "cpos": cpos, "cneg": cneg}


@pytest.mark.parametrize("tag", ["int", "flt"])
def test_G36_inputs_against_the_restatement(tag):
    d, stored = g36_case(tag)
    r = ref_of(d)
    got, left, right = run(d, return_windows=True)
    check(got, r, f"G36 {tag}")
    assert left.dtype == torch.int64 and np.array_equal(N(left), r["left"]) and np.array_equal(N(right), r["right"])
    for name, (gold, sel) in stored.items():           # and next to the reference's own float32 result: both within K u E of the same truth
        d2 = np.abs(N(got)[sel].astype(np.float64) - gold) / (R.U * r["E"][sel])
        print(f"G36 {tag} {name}: |kernel - reference| / (u E) worst {d2.max():.3f}")
        assert d2.max() <= 2 * R.K


def test_through_event_tables_and_into_the_batcher():
    """EventTables.from_arrays on raw arrays, compute_edi_prior on a shuffled subset of the exposures, ImageBatcher.set_pts0_prior"""
    from scipy.spatial.transform import Rotation as Rot      # test-side only: rotations for the key poses
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd import weights as W
    from evdeblurnerf_amd.events import EventTables
    from evdeblurnerf_amd.loader import ImageBatcher
    rs = np.random.RandomState(3611)
    h, w, n_ev, n_exp, M = 60, 80, 150_000, 7, 12
    act = rs.rand(h, w) < 0.9
    ys, xs = np.where(act)
    pick = rs.randint(0, ys.shape[0], n_ev)
    ex = (xs[pick] + 0.31 * np.sin(0.04 * ys[pick]) + 0.45).astype(np.float32)
    ey = (ys[pick] + 0.27 * np.cos(0.03 * xs[pick]) + 0.35).astype(np.float32)
    key_t = (np.arange(M) * 10_000 + 100_000).astype(np.int64)
    et = np.sort(rs.randint(key_t[0] - 5_000, key_t[-1] + 5_000, n_ev)).astype(np.int64)
    ep = rs.randint(0, 2, n_ev)
    Rk = Rot.from_rotvec(np.cumsum(rs.standard_normal((M, 3)) * 0.03, 0)).as_matrix()
    apb = np.concatenate([np.concatenate([Rk, rs.standard_normal((M, 3, 1)), np.ones((M, 3, 1))], -1).reshape(M, 15), np.ones((M, 2))], -1)
    mid = np.linspace(key_t[1], key_t[-2], n_exp)
    tb = EventTables.from_arrays(ex, ey, et, ep, h, w, key_t, apb, img_timestamps=mid, img_timestamps_start=mid - 2_400.0, img_timestamps_end=mid + 2_400.0,
                                 events_tms_unit="us", events_tms_files_unit="us", recenter=False)
    i_images = rs.permutation(n_exp)[:5]
    images = rs.uniform(0.02, 1.0, (5, h, w, 3)).astype(np.float32)
    prior = tb.compute_edi_prior(i_images, T(images), 9, 0.2, 0.25)
    assert prior.dtype == torch.float32 and prior.is_cuda and tuple(prior.shape) == images.shape
    d = {"events": N(tb.events), "id_to_coords": N(tb.id_to_coords), "tms_start": (mid - 2_400.0)[i_images], "tms_end": (mid + 2_400.0)[i_images],
         "images": images, "steps": 9, "cpos": 0.2, "cneg": 0.25}
    check(prior, ref_of(d), "EventTables.compute_edi_prior, 5 of 7 exposures shuffled")
    assert torch.equal(prior, tb.compute_edi_prior(torch.as_tensor(i_images), images, 9, 0.2, 0.25))
    # the consumer: the rows a batch serves are the prior's pixels bit for bit
    b = ImageBatcher(images, rs.standard_normal((5, 3, 4)).astype(np.float32), W.synthetic_camera())
    b.set_pts0_prior(prior)
    ids = T(rs.randint(0, len(b), 4096).astype(np.int64))
    out = b[ids]
    assert torch.equal(out["rgbsf_pts0"], prior.reshape(-1, 3)[ids]) and torch.equal(out["rgbsf"], T(images).reshape(-1, 3)[ids])
    # where the reference asserts
    bad = tb.images_timestamps_start.copy()
    for value in (tb.images_timestamps_end[2] + 1.0, 0.0):
        tb.images_timestamps_start = bad.copy()
        tb.images_timestamps_start[2] = value
        with pytest.raises(L.EvdError):
            tb.compute_edi_prior([2], images[:1], 9, 0.2, 0.25)
    tb.images_timestamps_start = None
    with pytest.raises(L.EvdError):
        tb.compute_edi_prior([2], images[:1], 9, 0.2, 0.25)


def test_bit_reproducible_whatever_the_chunking():
    d = stream(3621, 64, 96, 200_000, 5, hot=0.2)
    a = run(d)
    assert torch.equal(a, run(d))
    for c in (1, 2, 3):                                 # a workspace for c images: several chunks
        assert torch.equal(a, run(d, chunk=c)), c
    one = dict(d)
    for i in range(5):                                  # one image per call
        one.update(tms_start=d["tms_start"][i:i + 1], tms_end=d["tms_end"][i:i + 1], images=d["images"][i:i + 1])
        assert torch.equal(a[i:i + 1], run(one)), i
    many = stream(3622, 24, 32, 60_000, 37, exposure=1_600, gap=100)        # more images than the cap of a chunk
    m = run(many)
    check(m, ref_of(many), "37 images (three chunks of <= 16)")
    assert torch.equal(m, run(many, chunk=5))


@pytest.mark.parametrize("h,w", [(260, 346), (400, 400)])
def test_at_size(h, w):
    d = stream(3630 + h, h, w, 2_000_000, 8)
    r = ref_of(d)
    got, left, right = run(d, return_windows=True)
    check(got, r, f"{h} x {w}, 2 M events, 8 images")
    assert np.array_equal(N(left), r["left"]) and np.array_equal(N(right), r["right"])
    assert (r["right"][:, -1] - r["left"][:, 0]).min() > 100_000 and (r["right"][:, 1:-1] > r["left"][:, 1:-1]).any()       # events ON interior boundaries


@pytest.mark.parametrize("steps", [3, 5, 9, 17])
def test_steps_and_unequal_thresholds(steps):
    d = stream(3640 + steps, 40, 56, 40_000, 3, steps=steps, cpos=0.35, cneg=0.15, exposure=1_600 * 16, gap=500)
    check(run(d), ref_of(d), f"steps {steps}, c_pos 0.35, c_neg 0.15")


def test_edges():
    from evdeblurnerf_amd import _lib as L
    from evdeblurnerf_amd.edi import brightness_increment_image
    rs = np.random.RandomState(3651)
    h, w, steps = 12, 16, 9
    # exposure 0: windows 2 and 5 without events; exposure 1: no event at all
    start, end = np.array([10_000.0, 20_000.0]), np.array([10_800.0, 20_800.0])
    t = rs.randint(10_000, 10_801, 600)
    t = np.sort(t[~(((t >= 10_200) & (t <= 10_300)) | ((t >= 10_500) & (t <= 10_600)))]).astype(np.float64)       # (a window is closed on both sides)
    n_ev = len(t)
    coords = np.array([[w - 1.0, 3.0], [w - 0.5, 4.25], [2.5, h - 1.0], [3.25, h - 0.5], [-0.25, 5.5], [6.5, -0.125], [-0.5, -0.5], [-1.0, 2.0],
                       [w - 0.5, h - 0.5], [0.0, 0.0]] + [[rs.uniform(0, w - 1), rs.uniform(0, h - 1)] for _ in range(30)])
    i2c = coords.astype(np.float32).astype(np.float64)
    ev = np.stack([rs.randint(0, len(i2c), n_ev).astype(np.float64), t, rs.choice([-1.0, 1.0], n_ev), np.zeros(n_ev)], -1)
    images = rs.uniform(0.02, 1.0, (2, h, w, 3)).astype(np.float32)
    d = {"events": ev, "id_to_coords": i2c, "tms_start": start, "tms_end": end, "images": images, "steps": steps, "cpos": 0.2, "cneg": 0.3}
    r = ref_of(d)
    assert ((r["right"][0, 1:] - r["left"][0, :-1]) == 0).sum() == 2 and r["right"][1, -1] == r["left"][1, 0]
    got = run(d)
    check(got, r, "edges: empty windows, an empty exposure, last column / row, coordinates below 0")
    empty = np.abs(N(got)[1].astype(np.float64) - images[1]) / (R.U * r["E"][1])
    print(f"an exposure without events: |prior - image| / (u E) worst {empty.max():.3f}")
    assert empty.max() <= R.K
    # a coordinate slightly below 0: only its in-frame taps land, in the prior (above) and in the stand-alone splat with its guard
    x = np.array([-0.25, 6.5, -0.5, 3.0, w - 0.5], np.float32)
    y = np.array([5.5, -0.125, -0.5, 2.25, h - 0.5], np.float32)
    img = N(brightness_increment_image(T(x), T(y), T(np.ones(5, np.int8)), w, h, 0.2, 0.3))
    S, Nt = R.splat(x.astype(np.float64), y.astype(np.float64), h, w)
    want = float(np.float32(0.2)) * S.reshape(h, w)
    err = np.abs(img - want)
    print(f"brightness_increment_image with taps left of / above the frame: worst err {err.max():.2e}")
    assert np.all(err <= R.K * R.U * float(np.float32(0.2)) * (Nt * S + 2 * S).reshape(h, w)) and want[5, 0] > 0 and img[5, 0] > 0 and want[0, 6] > 0
    assert np.count_nonzero(img) == np.count_nonzero(want) == 2 + 2 + 1 + 2 + 1
    # a coordinate id outside the table is skipped and flagged
    bad = ev.copy()
    bad[7, 0], bad[40, 0] = len(i2c), -1.0
    with pytest.raises(L.EvdError):
        run(dict(d, events=bad))
    keep = np.ones(n_ev, bool)
    keep[[7, 40]] = False
    assert torch.equal(run(dict(d, events=bad), check=False), run(dict(d, events=ev[keep])))
