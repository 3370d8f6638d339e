"""Every form of the compositing scan (evd_raw2outputs, evd_raw2outputs_bwd_rays) and of the importance resampling (evd_sample_pdf_merge)
against the float64 reference of tests/composite_ref.py, element by element: |kernel - ref| <= K u E with u = 2^-24, E the reference's
first-order bound for the form, and isfinite(kernel) == isfinite(ref).  The forms are reached by shape and mode only, as the entries
dispatch them; each case id names the kernel it expects.

Error model (units of u; composite_ref.py derives each term, here is what differs between the forms):
  __expf in k_composite_il        exp2 of x log2(e): one more rounding of the argument, |x| relative on e (fast_exp); expf elsewhere
  act_fast (il, rows)             sigmoid = rcp(1 + __expf(-x)): 1 ulp reciprocal + 1 ulp exp2 + the add, and |x| (1 - s) from the
                                  argument: (5 + |x| (1 - s)) s, the same constant as the IEEE expf + division of act()
  product scan over S factors     one rounding per factor in any association (lane-local products, 6 DPP steps, the chunk carry) + 3
  sums over S                     roundings along any path: il NCH - 1 + 6 (chunks, then the 6-step DPP tree to lane 63), rows SPL - 1 + 7
                                  (samples per lane, 4 DPP steps + 3 row adds), k_composite ceil(S/64) - 1 + 6, k_weighted_channels S
  backward sigma gradient         the suffix sum_{j>i} G_j w_j is total - inclusive prefix: bounded by the WHOLE row's sum |G_j w_j|
  sample_pdf                      the knots and the index are bit-exact; t = (u - c0) / denom and b0 + t (b1 - b0): 5 |t (b1 - b0)| + |s|
K = 2 covers the second-order terms; an absolute 2^-120 covers float32 underflow.  z_merged and order are exact; z_std is a float64 evaluation rounded once.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from evdeblurnerf_amd import _lib as L
from composite_ref import cdf_knots, composite, composite_bwd, merge, sample_pdf_merge, z_std

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = 2.0
TINY = 2.0 ** -120       # float32 results below the normal range may be flushed to zero: an absolute allowance
DEV = "cuda"
A = L.ACT
LAYOUTS = {"nerf": (3, 0, "sigmoid"), "pdrf_coarse": (0, 1, "relu"), "pdrf_fine": (0, 1, "none")}
SC_NAME = {3: "3", 0: "0"}


def check(name, got, ref, E, k=K):
    got, ref, E = got.detach().double(), ref.detach().double().to(got.device), E.detach().double().to(got.device)
    fin = torch.isfinite(ref)
    gfin = torch.isfinite(got)
    assert torch.equal(gfin, fin), f"{name}: finiteness differs at {int((gfin != fin).sum())} elements, first {torch.nonzero(gfin != fin)[:4].tolist()}"
    bound = torch.where(torch.isfinite(E), k * U * E + TINY, torch.full_like(E, float("inf")))
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    bad = err > bound
    if bad.any():
        idx = torch.nonzero(bad)[:5]
        ratio = float((err / (U * E + 1e-300)).max())
        info = "; ".join(f"{tuple(i.tolist())}: got {float(got[tuple(i)]):.9g} ref {float(ref[tuple(i)]):.9g} E {float(E[tuple(i)]):.3g}" for i in idx)
        raise AssertionError(f"{name}: {int(bad.sum())} elements over {k} u E, worst err / (u E) = {ratio:.3g}: {info}")


def make_rays(R, S, C, sigma_ch, seed, sigma_act="relu", stride=3, dup_z=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    raw = torch.randn((R, S, C), generator=g, device=DEV)
    if sigma_act == "exp":
        off = torch.tensor([-20.0, -3.0, 0.0, 2.0], device=DEV)[torch.randint(0, 4, (R, 1), generator=g, device=DEV)]
        raw[..., sigma_ch] += off
    else:
        sc = torch.tensor([0.0, 0.5, 5.0, 50.0, 2000.0], device=DEV)[torch.randint(0, 5, (R, 1), generator=g, device=DEV)]
        raw[..., sigma_ch] *= sc
    z = torch.sort(2 + 4 * torch.rand((R, S), generator=g, device=DEV), -1)[0]
    if dup_z and S > 2:
        z[1::7, S // 2] = z[1::7, S // 2 - 1]                          # zero-width intervals
    rd = torch.randn((R, stride), generator=g, device=DEV)
    return raw.contiguous(), z.contiguous(), rd.contiguous()


def run_fwd(raw, z, rd, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, white=False, rmnear=0.0, noise=None, want=None, feature=None):
    R, S, Cc = raw.shape
    want = want or ("rgb", "acc", "weights", "depth", "density")
    shp = dict(rgb=(R, n_rgb), acc=(R,), weights=(R, S), depth=(R,), density=(R, max(S - 1, 1)))
    o = {k: torch.full(shp[k], float("nan"), device=DEV) for k in want}
    F = feature.shape[-1] if feature is not None else 0
    fmap = torch.full((R, F), float("nan"), device=DEV) if feature is not None else None
    L.check(L.lib().evd_raw2outputs(L.ptr(raw), L.ptr(z), L.ptr(rd), rd.shape[1], R, S, Cc, sigma_ch, rgb_ch0, n_rgb, A[rgb_act], A[sigma_act],
                                    int(white), rmnear, L.ptr(noise), L.ptr(o.get("rgb")), L.ptr(o.get("density")), L.ptr(o.get("acc")),
                                    L.ptr(o.get("weights")), L.ptr(o.get("depth")), L.ptr(feature), F, L.ptr(fmap), L.stream_ptr()),
            "evd_raw2outputs")
    torch.cuda.synchronize()
    if fmap is not None:
        o["fmap"] = fmap
    return o


def check_fwd(name, o, r, rows=None, S=None):
    sel = (lambda t: t[rows]) if rows is not None else (lambda t: t)
    for k in ("rgb", "acc", "depth", "weights", "fmap"):
        if k in o:
            check(f"{name} {k}", sel(o[k]), r[k], r["E_" + k])
    if "density" in o and S > 1:
        check(f"{name} density", sel(o["density"]), r["density"], r["E_density"])


def fwd_case(name, R, S, layout=None, sigma_ch=3, rgb_ch0=0, C=4, n_rgb=3, rgb_act="sigmoid", sigma_act="relu", white=False, rmnear=0.0,
             noise=False, form_name="il", seed=0, stride=3, feature=0, want=None, rows=None):
    if layout:
        sigma_ch, rgb_ch0, rgb_act = LAYOUTS[layout]
    raw, z, rd = make_rays(R, S, C, sigma_ch, seed, sigma_act, stride)
    nz = torch.randn((R, S - 1), device=DEV) if noise and S > 1 else None
    ft = torch.randn((R, S, feature), device=DEV) if feature else None
    o = run_fwd(raw, z, rd, sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, white, rmnear, nz, want, ft)
    if rows is None:
        rows = torch.arange(R, device=DEV)
    r = composite(raw[rows], z[rows], rd[rows], sigma_ch, rgb_ch0, n_rgb, rgb_act, sigma_act, white, rmnear,
                  None if nz is None else nz[rows], None if ft is None else ft[rows], form_name)
    check_fwd(name, o, r, rows, S)


def subset(R):
    """every row when R is small; otherwise the first 300, the last 261 (the ragged tail of 4 RPW) and 400 in between"""
    if R <= 1024:
        return None
    mid = torch.randperm(R - 561, generator=torch.Generator().manual_seed(R))[:400] + 300
    return torch.cat([torch.arange(300), mid, torch.arange(R - 261, R)]).to(DEV)


# ---- k_composite_il: all 36 instances -------------------------------------------------------------------------------------------
IL_S = {1: (33, 64), 2: (65, 128), 3: (129, 192), 4: (193, 256)}
IL_R = {1: 37, 2: 2 ** 14 + 5, 4: 2 ** 17 + 3}
RA_NAME = {"nerf": "sigmoid", "pdrf_coarse": "relu", "pdrf_fine": "none"}
IL_CASES = [(lay, nch, rpw) for lay in LAYOUTS for nch in (1, 2, 3, 4) for rpw in (1, 2, 4)]


@pytest.mark.parametrize("layout,nch,rpw", IL_CASES,
                         ids=[f"k_composite_il<{n},{p},{LAYOUTS[l][0]},{RA_NAME[l]},relu,true>-{l}" for l, n, p in IL_CASES])
def test_il_matches_float64(layout, nch, rpw):
    i = IL_CASES.index((layout, nch, rpw))
    R = IL_R[rpw]
    for S in IL_S[nch] if rpw == 1 else IL_S[nch][i % 2:i % 2 + 1]:
        fwd_case(f"il S={S} R={R}", R, S, layout, white=bool(i % 2), noise=i % 3 == 0, form_name="il", seed=i * 7 + S, rows=subset(R))


# ---- k_composite_rows SPL 1..4 ----------------------------------------------------------------------------------------------------
ROWS_MODES = {"rmnear": dict(rmnear=4.0), "softplus": dict(sigma_act="softplus"), "exp": dict(sigma_act="exp"),
              "sigmoid1": dict(rgb_act="sigmoid1"), "tanh": dict(rgb_act="tanh"),
              "layout_s0_sigmoid": dict(sigma_ch=0, rgb_ch0=1, rgb_act="sigmoid"), "layout_s3_relu": dict(rgb_act="relu")}
ROWS_CASES = [(m, spl) for m in ROWS_MODES for spl in (1, 2, 3, 4)]


@pytest.mark.parametrize("mode,spl", ROWS_CASES, ids=[f"k_composite_rows<{s},2>-{m}" for m, s in ROWS_CASES])
def test_rows_matches_float64(mode, spl):
    i = ROWS_CASES.index((mode, spl))
    for S in ((33, 64), (65, 128), (150, 192), (193, 256))[spl - 1]:
        fwd_case(f"rows {mode} S={S}", 37 + (i % 2), S, white=bool(i % 2), noise=i % 3 == 1, form_name="rows", seed=100 + i * 3 + S,
                 **ROWS_MODES[mode])


# ---- k_composite<3>, k_composite<0> + k_weighted_channels, feature maps ----------------------------------------------------------
@pytest.mark.parametrize("S,C,sc,c0", [(257, 4, 3, 0), (300, 4, 0, 1), (100, 5, 4, 1), (40, 6, 0, 2)],
                         ids=["k_composite<3>-S257", "k_composite<3>-S300-pdrf", "k_composite<3>-C5", "k_composite<3>-C6-rmnear"])
def test_composite3_matches_float64(S, C, sc, c0):
    for white in (False, True):
        fwd_case(f"composite<3> S={S} C={C}", 21, S, sigma_ch=sc, rgb_ch0=c0, C=C, white=white, noise=white, form_name="composite",
                 rmnear=4.0 if C == 6 else 0.0, seed=S + C)


@pytest.mark.parametrize("n_rgb,white", [(1, False), (1, True), (15, False), (15, True)],
                         ids=[f"k_composite<0>+k_weighted_channels-n_rgb{n}-{'white' if w else 'black'}" for n, w in [(1, 0), (1, 1), (15, 0), (15, 1)]])
def test_composite0_weighted_channels_matches_float64(n_rgb, white):
    for S in (64, 130):
        fwd_case(f"composite<0> n_rgb={n_rgb} S={S}", 19, S, sigma_ch=0, rgb_ch0=1, C=n_rgb + 1, n_rgb=n_rgb, rgb_act="relu", white=white,
                 form_name="weighted", seed=n_rgb + S)


@pytest.mark.parametrize("F,form_name", [(16, "il"), (300, "il"), (16, "rows"), (300, "composite")],
                         ids=["k_composite_il+k_weighted_channels<64>-F16", "k_composite_il+k_weighted_channels<256>-F300",
                              "k_composite_rows+k_weighted_channels<64>-F16", "k_composite<3>+k_weighted_channels<256>-F300"])
def test_feature_maps_match_float64(F, form_name):
    S = {"il": 96, "rows": 96, "composite": 270}[form_name]
    fwd_case(f"fmap F={F}", 23, S, layout="nerf", rmnear=4.0 if form_name == "rows" else 0.0, feature=F, form_name=form_name, seed=F)


# ---- the C ABI: strided ray rows, optional outputs --------------------------------------------------------------------------------
CABI = [("il", dict(layout="nerf")), ("rows", dict(sigma_act="softplus")), ("composite", dict(C=5, sigma_ch=4, rgb_ch0=1))]
CABI_IDS = {"il": "k_composite_il<2,1,3,sigmoid,relu,true>", "rows": "k_composite_rows<2,2>", "composite": "k_composite<3>"}


@pytest.mark.parametrize("form_name", [c[0] for c in CABI], ids=[CABI_IDS[c[0]] for c in CABI])
def test_cabi_stride11_noise_density_and_null_outputs(form_name):
    kw = dict(CABI)[form_name]
    fwd_case(f"{form_name} stride 11 + noise", 29, 100, stride=11, noise=True, form_name=form_name, seed=5, **kw)
    for want in (("rgb",), ("weights",), ("acc", "depth"), ("density",)):
        fwd_case(f"{form_name} only {want}", 29, 100, stride=11, noise=True, want=want, form_name=form_name, seed=6, **kw)


# ---- input edges -------------------------------------------------------------------------------------------------------------------
EDGE_FORMS = {"k_composite_il": dict(layout="nerf", form_name="il"),
              "k_composite_rows": dict(sigma_act="softplus", form_name="rows"),
              "k_composite<3>": dict(C=5, sigma_ch=4, rgb_ch0=1, form_name="composite")}


@pytest.mark.parametrize("kernel", list(EDGE_FORMS), ids=list(EDGE_FORMS))
def test_input_edges(kernel):
    """empty rays, an opaque first sample, duplicate z, softplus past its threshold, S in {1, 2}"""
    kw = dict(EDGE_FORMS[kernel])
    form_name = kw.pop("form_name")
    layout = kw.pop("layout", None)
    sigma_ch, rgb_ch0 = (LAYOUTS[layout][0], LAYOUTS[layout][1]) if layout else (kw.get("sigma_ch", 3), kw.get("rgb_ch0", 0))
    rgb_act = LAYOUTS[layout][2] if layout else "sigmoid"
    sigma_act = kw.get("sigma_act", "relu")
    Cc = kw.get("C", 4)
    for S in (1, 2, 3, 64, 65):
        R = 24
        raw, z, rd = make_rays(R, S, Cc, sigma_ch, S, sigma_act)
        raw[0:4, :, sigma_ch] = 0.0                                   # empty rays
        raw[4:8, 0, sigma_ch] = 1e6                                   # opaque first sample
        raw[8:12, :, sigma_ch] = 25.0 + 10 * torch.rand((4, S), device=DEV)      # softplus past 20 (x - 1 > 20)
        z[12:16] = z[12:16, :1].expand(-1, S).contiguous()            # every interval of zero width
        z[16:20, 1::2] = z[16:20, 0:-1:2][:, :z[16:20, 1::2].shape[1]]
        o = run_fwd(raw, z, rd, sigma_ch, rgb_ch0, 3, rgb_act, sigma_act)
        r = composite(raw, z, rd, sigma_ch, rgb_ch0, 3, rgb_act, sigma_act, form_name=form_name)
        check_fwd(f"{kernel} edges S={S}", o, r, None, S)
        assert torch.allclose(o["acc"][0:4], torch.ones(4, device=DEV), atol=1e-6)      # the last alpha is 1


# ---- finiteness: NaN and +-Inf planted in sigma and colour ---------------------------------------------------------------------
NAN_FORMS = [("k_composite_il<2,1,3,sigmoid,relu,true>", dict(layout="nerf", form_name="il", S=100)),
             ("k_composite_il<2,1,0,relu,relu,true>", dict(layout="pdrf_coarse", form_name="il", S=100)),
             ("k_composite_il<4,1,0,none,relu,true>", dict(layout="pdrf_fine", form_name="il", S=250)),
             ("k_composite_rows<2,2>", dict(rmnear=2.5, layout="pdrf_coarse", form_name="rows", S=100)),
             ("k_composite<3>", dict(layout="pdrf_coarse", form_name="composite", S=300)),
             ("k_composite<0>+k_weighted_channels", dict(C=16, n_rgb=15, sigma_ch=0, rgb_ch0=1, rgb_act="relu", form_name="weighted", S=70))]


@pytest.mark.parametrize("kernel,kw", NAN_FORMS, ids=[f[0] for f in NAN_FORMS])
def test_nan_and_inf_propagate_as_in_the_reference(kernel, kw):
    kw = dict(kw)
    S, form_name = kw.pop("S"), kw.pop("form_name")
    layout = kw.pop("layout", None)
    sigma_ch, rgb_ch0, rgb_act = LAYOUTS[layout] if layout else (kw.pop("sigma_ch"), kw.pop("rgb_ch0"), kw.pop("rgb_act"))
    Cc, n_rgb, rmnear = kw.get("C", 4), kw.get("n_rgb", 3), kw.get("rmnear", 0.0)
    R = 32
    raw, z, rd = make_rays(R, S, Cc, sigma_ch, 77, dup_z=False)
    raw[..., sigma_ch] = 0.3 * raw[..., sigma_ch].abs()               # no weight underflows to 0 behind a planted value
    cols = [c for c in range(rgb_ch0, rgb_ch0 + n_rgb)]
    pos = [0, 1, 63, 64, S // 2, S - 2, S - 1]
    vals = [float("nan"), float("inf"), float("-inf")]
    row = 0
    for p in pos:
        for v in vals:
            raw[row, p, sigma_ch] = v
            raw[row + 1, p, cols[row % len(cols)]] = v
            row += 2
            if row >= R - 2:
                break
        if row >= R - 2:
            break
    o = run_fwd(raw, z, rd, sigma_ch, rgb_ch0, n_rgb, rgb_act, "relu", rmnear=rmnear)
    r = composite(raw, z, rd, sigma_ch, rgb_ch0, n_rgb, rgb_act, "relu", rmnear=rmnear, form_name=form_name)
    check_fwd(f"{kernel} planted", o, r, None, S)
    assert not torch.isfinite(r["acc"]).all()                          # the planted values do reach the outputs


# ---- backward: k_composite_rows_bwd ---------------------------------------------------------------------------------------------
BWD_PAIRS = [("nerf", "sigmoid", "relu"), ("nerf", "relu", "relu"), ("nerf", "none", "relu"), ("nerf", "exp", "relu"),
             ("nerf", "sigmoid1", "relu"), ("nerf", "softplus", "relu"), ("nerf", "sigmoid", "softplus"), ("nerf", "sigmoid", "exp"),
             ("nerf", "sigmoid", "sigmoid"), ("nerf", "sigmoid", "sigmoid1"), ("pdrf", "relu", "relu"), ("pdrf", "none", "relu"),
             ("pdrf", "tanh", "relu"), ("pdrf", "none", "softplus")]
BWD_CASES = [(l, ra, sa, spl) for l, ra, sa in BWD_PAIRS for spl in (1, 2, 3, 4)]
BWD_S = {1: (33, 64), 2: (65, 128), 3: (129, 192), 4: (193, 256)}


def run_bwd(raw, z, rd, sc, c0, ra, sa, white, rmnear, noise, g, d_stride=3):
    R, S, Cc = raw.shape
    d_raw = torch.full_like(raw, float("nan"))
    d_rd = torch.full((R, d_stride), 1234.5, device=DEV) if d_stride else None
    gg = [None if t is None else t.contiguous() for t in g]
    L.check(L.lib().evd_raw2outputs_bwd_rays(L.ptr(raw), L.ptr(z), L.ptr(rd), rd.shape[1], R, S, Cc, sc, c0, 3, A[ra], A[sa], int(white), rmnear,
                                             L.ptr(noise), L.ptr(gg[0]), L.ptr(gg[1]), L.ptr(gg[2]), L.ptr(gg[3]), L.ptr(d_raw), L.ptr(d_rd),
                                             d_stride, L.stream_ptr()), "evd_raw2outputs_bwd_rays")
    torch.cuda.synchronize()
    return d_raw, d_rd


def bwd_case(name, R, S, layout, ra, sa, white=False, rmnear=0.0, noise=False, drop=None, stride=3, d_stride=3, seed=0):
    sc, c0 = (3, 0) if layout == "nerf" else (0, 1)
    raw, z, rd = make_rays(R, S, 4, sc, seed, sa, stride)
    if sa == "relu" or sa == "softplus":
        raw[..., sc] = raw[..., sc].clamp(max=200.0)
    nz = torch.randn((R, S - 1), device=DEV) if noise else None
    gs = [torch.randn(sh, device=DEV) for sh in ((R, 3), (R,), (R,), (R, S))]
    g = [None if i == drop else gs[i] for i in range(4)]
    d_raw, d_rd = run_bwd(raw, z, rd, sc, c0, ra, sa, white, rmnear, nz, g, d_stride)
    r = composite_bwd(raw, z, rd, *g, sigma_ch=sc, rgb_ch0=c0, rgb_act=ra, sigma_act=sa, white=white, rmnear=rmnear, noise=nz)
    check(f"{name} d_raw", d_raw, r["d_raw"], r["E_d_raw"])
    if d_stride:
        check(f"{name} d_rays_d", d_rd[:, :3], r["d_rays_d"], r["E_d_rays_d"])
        assert (d_rd[:, 3:] == 1234.5).all(), f"{name}: d_rays_d written past column 2"


@pytest.mark.parametrize("layout,ra,sa,spl", BWD_CASES, ids=[f"k_composite_rows_bwd<{s}>-{l}-{ra}-{sa}" for l, ra, sa, s in BWD_CASES])
def test_bwd_matches_float64(layout, ra, sa, spl):
    i = BWD_CASES.index((layout, ra, sa, spl))
    S = BWD_S[spl][i % 2]
    bwd_case(f"bwd S={S}", 33, S, layout, ra, sa, white=bool(i % 3 == 1), seed=300 + i)


BWD_MODES = [("white", dict(white=True)), ("rmnear", dict(rmnear=4.0)), ("noise", dict(noise=True)), ("no_g_map", dict(drop=0)),
             ("no_g_depth", dict(drop=1)), ("no_g_acc", dict(drop=2)), ("no_g_weights", dict(drop=3)), ("rays_d_stride11", dict(stride=11, d_stride=11)),
             ("no_d_rays_d", dict(d_stride=0))]
BWD_MODE_CASES = [(m, kw, spl) for m, kw in BWD_MODES for spl in (1, 4)]


@pytest.mark.parametrize("mode,kw,spl", BWD_MODE_CASES, ids=[f"k_composite_rows_bwd<{s}>-{m}" for m, _, s in BWD_MODE_CASES])
def test_bwd_modes_match_float64(mode, kw, spl):
    for layout in ("nerf", "pdrf"):
        ra = "sigmoid" if layout == "nerf" else "none"
        bwd_case(f"bwd {mode} {layout}", 35, (50, 256)[spl == 4], layout, ra, "relu", seed=len(mode) * 13 + spl, **kw)


def test_bwd_refuses_s_over_256_and_c_not_4():
    for S, Cc in ((257, 4), (64, 5)):
        raw, z, rd = make_rays(3, S, Cc, 3, 1)
        d_raw = torch.empty_like(raw)
        with pytest.raises(L.EvdError):
            L.check(L.lib().evd_raw2outputs_bwd_rays(L.ptr(raw), L.ptr(z), L.ptr(rd), 3, 3, S, Cc, 3, 0, 3, A["sigmoid"], A["relu"], 0, 0.0, None,
                                                     None, None, None, None, L.ptr(d_raw), None, 3, L.stream_ptr()), "bwd")


# ---- k_sample_pdf_merge ---------------------------------------------------------------------------------------------------------
PDF_S = [3, 4, 17, 64, 65, 128, 129, 256]
PDF_N = [1, 2, 63, 64, 65, 128, 192]


def pdf_inputs(R, S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.sort(1 + 5 * torch.rand((R, S), generator=g, device=DEV), -1)[0]
    z[1::5, S // 2] = z[1::5, S // 2 - 1]                              # duplicate z
    z[2::9] = z[2::9, :1].expand(-1, S)                                # every z equal
    w = torch.rand((R, S), generator=g, device=DEV) ** 4
    w[3::6] = 0                                                        # all zero: uniform pdf
    w[4::6] = 0
    w[4::6, S // 2] = 1                                                # one-hot: the denom guard everywhere else
    w[5::6] *= 1e-30
    return z.contiguous(), w.contiguous()


def run_pdf(z, w, N, det, u):
    R, S = z.shape
    zs = torch.full((R, N), float("nan"), device=DEV)
    zm = torch.full((R, S + N), float("nan"), device=DEV)
    order = torch.full((R, S + N), -1, dtype=torch.int32, device=DEV)
    zstd = torch.full((R,), float("nan"), device=DEV)
    L.check(L.lib().evd_sample_pdf_merge(L.ptr(z), L.ptr(w), R, S, N, int(det), L.ptr(u), L.ptr(zs), L.ptr(zm), L.ptr(order), L.ptr(zstd),
                                         L.stream_ptr()), "evd_sample_pdf_merge")
    torch.cuda.synchronize()
    return zs, zm, order, zstd


def knot_u(z, w, N, rs):
    """u on the float32 cdf knots, one float32 ulp either side of them, 0 and 1 -- N per ray"""
    c = cdf_knots(w[:, 1:-1]).cpu().numpy()
    cand = np.concatenate([c, np.nextafter(c, np.float32(-1)), np.nextafter(c, np.float32(2)), np.zeros_like(c[:, :1]), np.ones_like(c[:, :1])], 1)
    cand = np.clip(cand, 0, 1).astype(np.float32)
    idx = np.stack([rs.permutation(cand.shape[1])[:N] if cand.shape[1] >= N else rs.randint(0, cand.shape[1], N) for _ in range(z.shape[0])])
    u = np.take_along_axis(cand, idx, 1)
    u[:, 0] = 0.0
    if N > 1:
        u[:, 1] = 1.0
    return torch.tensor(np.ascontiguousarray(u), device=DEV)


@pytest.mark.parametrize("S", PDF_S, ids=[f"k_sample_pdf_merge-S{s}" for s in PDF_S])
def test_sample_pdf_merge_matches_float64(S):
    rs = np.random.RandomState(S)
    for N in PDF_N:
        R = 37 + N % 5
        z, w = pdf_inputs(R, S, S * 1000 + N)
        for tag, det, u in (("det", True, None), ("rand", False, torch.rand((R, N), device=DEV)), ("knots", False, knot_u(z, w, N, rs))):
            zs, zm, order, zstd = run_pdf(z, w, N, det, u)
            r = sample_pdf_merge(z, w, N, det=det, u=u)
            check(f"S={S} N={N} {tag} z_samples", zs, r["z_samples"], r["E_z_samples"])
            m, o = merge(z, zs)
            assert np.array_equal(zm.cpu().numpy(), m), f"S={S} N={N} {tag}: z_merged"
            assert np.array_equal(order.cpu().numpy(), o), f"S={S} N={N} {tag}: order is not the stable rank"
            sd = z_std(zs)
            check(f"S={S} N={N} {tag} z_std", zstd, sd, sd.abs() + 2.0 ** -20 * zs.double().abs().max(-1)[0])
