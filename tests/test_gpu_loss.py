"""The loss-side kernels (csrc/kernels_loss.hip; the AWP scan in csrc/kernel_awp_integrate.hip + awp_integrate.h) against the float64 reference of tests/loss_ref.py, element by element:
|kernel - ref| <= K u E with u = 2^-24, E the reference's first-order bound for the kernel form, K = 2 for the second-order terms, an absolute
2^-120 for float32 underflow, and isfinite(kernel) == isfinite(ref).  Every kernel form is reached by shape and mode alone through the
public entries; each case id names the kernel it expects.  Each case prints its worst err / (u E) before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from evdeblurnerf_amd import _lib as L
from evdeblurnerf_amd.tonemapping import CRF
import loss_ref as LR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = 2.0
TINY = 2.0 ** -120
DEV = "cuda"


def check(name, got, ref, E, k=K):
    """tests/test_gpu_composite.py's check(); prints the worst ratio"""
    got, ref, E = got.detach().double(), ref.detach().double().to(got.device).reshape(got.shape), E.detach().double().to(got.device).reshape(got.shape)
    fin = torch.isfinite(ref)
    gfin = torch.isfinite(got)
    assert torch.equal(gfin, fin), f"{name}: finiteness differs at {int((gfin != fin).sum())} elements, first {torch.nonzero(gfin != fin)[:4].tolist()}"
    bound = torch.where(torch.isfinite(E), k * U * E + TINY, torch.full_like(E, float("inf")))
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    ratio = float((torch.where(torch.isfinite(E), err, torch.zeros_like(err)) / (U * E + TINY)).max()) if err.numel() else 0.0
    print(f"[loss-f64] {name}: worst err / (u E) = {ratio:.3g} over {err.numel()} elements")
    bad = err > bound
    if bad.any():
        idx = torch.nonzero(bad)[:5]
        info = "; ".join(f"{tuple(i.tolist())}: got {float(got[tuple(i)]):.9g} ref {float(ref[tuple(i)]):.9g} E {float(E[tuple(i)]):.3g}" for i in idx)
        raise AssertionError(f"{name}: {int(bad.sum())} elements over {k} u E, worst err / (u E) = {ratio:.3g}: {info}")


# ---- evd_awp_feature_integration / _bwd -------------------------------------------------------------------------------------------
AWP_C = [1, 20, 63, 64, 65, 100, 128, 129, 200, 256]
AWP_S = [1, 2, 3, 5, 8, 9, 33, 128, 129]
AWP_N = [1, 3, 4, 5, 15, 16, 17, 33]
SCALES = [0.0, 0.05, 1.0, 8.0, 300.0]


def awp_kernel(C_, bwd=False):
    f = LR.awp_form(C_)["name"]
    return ("k_awp_integrate_bwd" if bwd else "k_awp_integrate") + ("_c64" if f == "c64" else f)


def awp_shapes(C_):
    """the pruned cross: every S once, N rotating (so every C meets ragged S and ragged N); C = 64 also with N = 1, 15, 17 at a ragged S"""
    i = AWP_C.index(C_)
    sh = [(AWP_N[(i + 3 * j) % len(AWP_N)], S) for j, S in enumerate(AWP_S)]
    if C_ == 64:
        sh += [(1, 9), (15, 5), (17, 33), (1, 1), (17, 2)]
    return sh


def awp_inputs(N, S, C_, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    sc = torch.tensor(SCALES, device=DEV)[torch.randint(0, 5, (N, 1, 1), generator=g, device=DEV)]
    if N >= 5:
        sc[:5, 0, 0] = torch.tensor(SCALES, device=DEV)                   # every scale present
    feat = torch.randn((N, S, C_), generator=g, device=DEV).abs() * sc
    z = torch.sort(2 + 4 * torch.rand((N, S), generator=g, device=DEV), -1)[0]
    if S > 2:
        z[1::3, S // 2] = z[1::3, S // 2 - 1]                              # zero-width intervals
    rd = torch.randn((N, 3), generator=g, device=DEV)
    if N > 2:
        rd[N // 2] = 0.0                                                   # a zero direction
    d_out = torch.randn((N, C_), generator=g, device=DEV)
    return feat.contiguous(), z.contiguous(), rd.contiguous(), d_out.contiguous()


def awp_fwd(feat, z, rd):
    N, S, C_ = feat.shape
    out = torch.full((N, C_), float("nan"), device=DEV)
    L.check(L.lib().evd_awp_feature_integration(L.ptr(feat), L.ptr(z), L.ptr(rd), N, S, C_, L.ptr(out), L.stream_ptr()), "evd_awp_feature_integration")
    torch.cuda.synchronize()
    return out


def awp_bwd(feat, z, rd, d_out, want_z=True, want_d=True):
    N, S, C_ = feat.shape
    d_feat = torch.full_like(feat, float("nan"))
    d_z = torch.full((N, S), 1234.5, device=DEV)
    d_rd = torch.full((N, 3), 1234.5, device=DEV)
    L.check(L.lib().evd_awp_feature_integration_bwd(L.ptr(feat), L.ptr(z), L.ptr(rd), L.ptr(d_out), N, S, C_, L.ptr(d_feat), L.ptr(d_z) if want_z else None,
                                                    L.ptr(d_rd) if want_d else None, L.stream_ptr()), "evd_awp_feature_integration_bwd")
    torch.cuda.synchronize()
    return d_feat, d_z, d_rd


def check_awp_bwd(name, got, r, want_z=True, want_d=True, rows=None):
    sel = (lambda t: t[rows]) if rows is not None else (lambda t: t)
    d_feat, d_z, d_rd = got
    check(f"{name} d_feat", sel(d_feat), r["d_feat"], r["E_d_feat"])
    if want_z:
        check(f"{name} d_z", sel(d_z), r["d_z"], r["E_d_z"])
    else:
        assert (d_z == 1234.5).all(), f"{name}: d_z written though NULL was passed"
    if want_d:
        check(f"{name} d_rays_d", sel(d_rd), r["d_rays_d"], r["E_d_rays_d"])
    else:
        assert (d_rd == 1234.5).all(), f"{name}: d_rays_d written though NULL was passed"


@pytest.mark.parametrize("C_", AWP_C, ids=[f"{awp_kernel(c)}-C{c}" for c in AWP_C])
def test_awp_forward_matches_float64(C_):
    for N, S in awp_shapes(C_):
        feat, z, rd, _ = awp_inputs(N, S, C_, 1000 * C_ + 10 * S + N)
        v, E = LR.awp_integrate(feat, z, rd)
        check(f"{awp_kernel(C_)} C={C_} N={N} S={S} out", awp_fwd(feat, z, rd), v, E)


@pytest.mark.parametrize("C_", AWP_C, ids=[f"{awp_kernel(c, True)}-C{c}" for c in AWP_C])
def test_awp_backward_matches_float64(C_):
    for j, (N, S) in enumerate(awp_shapes(C_)):
        feat, z, rd, d_out = awp_inputs(N, S, C_, 2000 * C_ + 10 * S + N)
        r = LR.awp_integrate_bwd(feat, z, rd, d_out)
        combos = [(True, True), (False, True), (True, False), (False, False)] if j in (3, 6) else [(True, True)]      # S = 5 and 33
        for want_z, want_d in combos:
            got = awp_bwd(feat, z, rd, d_out, want_z, want_d)
            check_awp_bwd(f"{awp_kernel(C_, True)} C={C_} N={N} S={S} d_z={int(want_z)} d_rays_d={int(want_d)}", got, r, want_z, want_d)


def test_awp_rejects_257_channels():
    feat, z, rd, d_out = awp_inputs(3, 4, 257, 1)
    with pytest.raises(L.EvdError):
        awp_fwd(feat, z, rd)
    with pytest.raises(L.EvdError):
        awp_bwd(feat, z, rd, d_out)


def test_awp_shipped_shape_k_awp_integrate_c64_and_bwd_c64():
    """10 240 rays x 128 samples x 64 channels: the kernels run on every ray, the reference on the first 200, the last 200 and 200 between"""
    N, S, C_ = 10240, 128, 64
    feat, z, rd, d_out = awp_inputs(N, S, C_, 77)
    rows = torch.cat([torch.arange(200), torch.randperm(N - 400, generator=torch.Generator().manual_seed(3))[:200] + 200, torch.arange(N - 200, N)]).to(DEV)
    v, E = LR.awp_integrate(feat[rows], z[rows], rd[rows])
    check("k_awp_integrate_c64 shipped out", awp_fwd(feat, z, rd)[rows], v, E)
    r = LR.awp_integrate_bwd(feat[rows], z[rows], rd[rows], d_out[rows])
    check_awp_bwd("k_awp_integrate_bwd_c64 shipped", awp_bwd(feat, z, rd, d_out), r, rows=rows)


# ---- evd_weighted_sum ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 3, 64, 65], ids=[f"k_weighted_sum-C{c}" for c in (1, 3, 64, 65)])
def test_weighted_sum_matches_float64(C_):
    g = torch.Generator(device=DEV).manual_seed(C_)
    for P in (1, 10, 16):
        for R in sorted({1, 7, 255 // C_ + 1, 256 // C_, 256 // C_ + 1, 1024}):       # R C below, on and above one 256-lane block
            if R < 1:
                continue
            x = torch.randn((R, P, C_), generator=g, device=DEV)
            w = torch.randn((R, P), generator=g, device=DEV)
            out = torch.full((R, C_), float("nan"), device=DEV)
            L.check(L.lib().evd_weighted_sum(L.ptr(x), L.ptr(w), R, P, C_, L.ptr(out), L.stream_ptr()), "evd_weighted_sum")
            torch.cuda.synchronize()
            v, E = LR.weighted_sum(x, w)
            check(f"k_weighted_sum C={C_} P={P} R={R}", out, v, E)


# ---- evd_blur_loss_reduce / evd_blur_loss_bwd{,_dev} ---------------------------------------------------------------------------------
BLUR_R = [1, 21, 22, 64, 257, 1024]
BLUR_P = [1, 5, 10, 16]
PRESENCE = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]          # rgb0_p, w2, target_pts0
_CRFS = {}


def crf_of(kind):
    """'none', 'gamma', 'learn' (make_crf_state_dict(51, 0): the image branch has no extra features)"""
    if kind not in _CRFS:
        from evdeblurnerf_amd import weights as W
        _CRFS[kind] = CRF("learn", state_dict=W.make_crf_state_dict(51, 0)) if kind == "learn" else CRF(kind)
    return _CRFS[kind]


def blur_inputs(R, P, seed, zero_rows):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rgb_p = 0.02 + 0.98 * torch.rand((R, P, 3), generator=g, device=DEV)
    rgb0_p = 0.02 + 0.98 * torch.rand((R, P, 3), generator=g, device=DEV)
    w = torch.sigmoid(torch.randn((2, R, P), generator=g, device=DEV))
    w = w / w.sum(-1, keepdim=True)
    if zero_rows and R > 2:
        w[:, 1::5] = 0.0                                                   # rows of all-zero weights
    tgt, tgt0 = torch.rand((R, 3), generator=g, device=DEV), torch.rand((R, 3), generator=g, device=DEV)
    return rgb_p.contiguous(), rgb0_p.contiguous(), w[0].contiguous(), w[1].contiguous(), tgt, tgt0


def blur_fwd(crf, skip, rgb_p, rgb0_p, w1, w2, tgt, tgt0, partial, colours):
    R, P = w1.shape
    cols = {k: torch.full((R, 3), 1234.5, device=DEV) for k in ("rgb", "rgb1", "rgb_awp")} if colours else {}
    L.check(L.lib().evd_blur_loss_reduce(crf.handle, int(skip), L.ptr(rgb_p), L.ptr(rgb0_p), L.ptr(w1), L.ptr(w2), L.ptr(tgt), L.ptr(tgt0), R, P,
                                         L.ptr(partial), L.ptr(cols.get("rgb")), L.ptr(cols.get("rgb1")), L.ptr(cols.get("rgb_awp")), L.stream_ptr()),
            "evd_blur_loss_reduce")
    torch.cuda.synchronize()
    return cols


def blur_bwd(crf, skip, rgb_p, rgb0_p, w1, w2, tgt, tgt0, g, dev_entry):
    R, P = w1.shape
    o = dict(d_rgb_p=torch.full_like(rgb_p, float("nan")), d_rgb0_p=torch.full_like(rgb_p, 1234.5), d_w1=torch.full_like(w1, float("nan")),
             d_w2=torch.full_like(w1, 1234.5))
    args = (crf.handle, int(skip), L.ptr(rgb_p), L.ptr(rgb0_p), L.ptr(w1), L.ptr(w2), L.ptr(tgt), L.ptr(tgt0), R, P)
    outs = (L.ptr(o["d_rgb_p"]), L.ptr(o["d_rgb0_p"]), L.ptr(o["d_w1"]), L.ptr(o["d_w2"]), L.stream_ptr())
    if dev_entry:
        gd = torch.tensor(g, dtype=torch.float32, device=DEV)
        L.check(L.lib().evd_blur_loss_bwd_dev(*args, L.ptr(gd), *outs), "evd_blur_loss_bwd_dev")
    else:
        gh = np.ascontiguousarray(g, dtype=np.float32)
        L.check(L.lib().evd_blur_loss_bwd(*args, gh.ctypes.data_as(C.POINTER(C.c_float)), *outs), "evd_blur_loss_bwd")
    torch.cuda.synchronize()
    return o


def blur_case(name, kind, skip, R, P, pres, seed, colours=True, partial0=False, dev_entry=False, backward=True, zero_rows=None, zero_colour=False):
    map_type = kind
    zero_rows = (kind != "gamma") if zero_rows is None else zero_rows
    rgb_p, rgb0_p, w1, w2, tgt, tgt0 = blur_inputs(R, P, seed, zero_rows)
    if zero_colour:
        rgb_p[0, :, 1] = 0.0                                               # pixel 0, green: a = c = 0 exactly, and the pts0 colour too
    has0, has2, hast = pres
    a0, a2, at = (rgb0_p if has0 else None), (w2 if has2 else None), (tgt0 if hast else None)
    p0 = torch.tensor([0.5, -2.0, 3.0, 0.25, 7.0, 12.0, 99.0, 98.0], device=DEV) if partial0 else torch.zeros(8, device=DEV)
    partial = p0.clone()
    cols = blur_fwd(crf_of(kind), skip, rgb_p, a0, w1, a2, tgt, at, partial, colours)
    r = LR.blur_loss(rgb_p, w1, tgt, rgb0_p=a0, w2=a2, tgt0=at, map_type=map_type, skip_learn=skip, partial0=p0[:6] if partial0 else None)
    check(f"{name} partial[0:5]", partial[:5], r["partial"][:5], r["E_partial"][:5])
    assert float(partial[5]) == 3 * R + float(p0[5]), f"{name}: partial[5] = {float(partial[5])}, expected exactly {3 * R + float(p0[5])}"
    assert torch.equal(partial[6:], p0[6:]), f"{name}: partial[6:8] touched"
    for k, present in (("rgb", True), ("rgb1", has0), ("rgb_awp", has2)):
        if colours and present:
            check(f"{name} {k}", cols[k], r[k], r["E_" + k])
        elif colours:
            assert (cols[k] == 1234.5).all(), f"{name}: {k} written without its input"
    if not backward:
        return
    g = [float(np.float32(v)) for v in (0.7, -1.3, 0.45, 2.1, -0.6)]           # the float32 numbers the kernel receives
    o = blur_bwd(crf_of(kind), skip, rgb_p, a0, w1, a2, tgt, at, g, dev_entry)
    rb = LR.blur_loss_bwd(rgb_p, w1, tgt, g, rgb0_p=a0, w2=a2, tgt0=at, map_type=map_type, skip_learn=skip)
    for k in ("d_rgb_p", "d_rgb0_p", "d_w1", "d_w2"):
        if k in rb:
            check(f"{name} {k}", o[k], rb[k], rb["E_" + k])
        elif k == "d_rgb0_p":
            assert (o[k] == 1234.5).all(), f"{name}: {k} written without its input"
        else:                                                              # d_w2 without w2: zeroed by the entry, nothing added
            assert (o[k] == 0).all(), f"{name}: {k} not zero without w2"
    if zero_colour:
        assert not torch.isfinite(rb["d_rgb_p"][0, :, 1]).any() and torch.isfinite(partial[:5]).all()


BLUR_KINDS = [("none", False), ("gamma", False), ("learn", True)]


@pytest.mark.parametrize("kind,skip", BLUR_KINDS, ids=[f"k_blur_loss+k_blur_loss_bwd-{k}{'-skip_learn' if s else ''}" for k, s in BLUR_KINDS])
def test_blur_loss_matches_float64(kind, skip):
    i = 0
    for R in BLUR_R:
        for P in BLUR_P:
            pres = PRESENCE[i % 8] if (R, P) != (1024, 10) else (1, 1, 1)
            blur_case(f"blur {kind} R={R} P={P} presence={pres}", kind, skip, R, P, pres, seed=100 * R + P, colours=i % 2 == 0, partial0=i % 3 == 0,
                      dev_entry=i % 2 == 1)
            i += 1


@pytest.mark.parametrize("pres", PRESENCE, ids=[f"k_blur_loss+k_blur_loss_bwd-rgb0_p{a}-w2{b}-target_pts0{c}" for a, b, c in PRESENCE])
def test_blur_loss_every_presence_combination(pres):
    for kind, skip in BLUR_KINDS:
        for dev_entry in (False, True):
            blur_case(f"blur {kind} presence={pres} dev={int(dev_entry)}", kind, skip, 257, 10, pres, seed=sum(pres) + 11, dev_entry=dev_entry)
            blur_case(f"blur {kind} presence={pres} dev={int(dev_entry)} no colours", kind, skip, 22, 5, pres, seed=sum(pres) + 12, colours=False,
                      dev_entry=dev_entry)


def test_blur_loss_gamma_exact_zero_colour_k_blur_loss_bwd():
    """a colour that is exactly 0 under gamma: the forward is finite (0^(1/2.2) = 0), the backward's 0^(1/2.2 - 1) is not, in the kernel
    and in the reference alike"""
    for dev_entry in (False, True):
        blur_case("blur gamma zero colour", "gamma", False, 22, 5, (1, 1, 1), seed=5, dev_entry=dev_entry, zero_rows=False, zero_colour=True)


def test_blur_loss_bwd_rejects_a_live_learn_crf():
    rgb_p, rgb0_p, w1, w2, tgt, tgt0 = blur_inputs(5, 3, 1, False)
    for dev_entry in (False, True):
        with pytest.raises(L.EvdError):
            blur_bwd(crf_of("learn"), False, rgb_p, rgb0_p, w1, w2, tgt, tgt0, [1.0] * 5, dev_entry)


# ---- a live learn CRF: inputs that clear the ReLU condition ---------------------------------------------------------------------------
def draw_safe(name, n, draw, safe_of):
    """draw ~1.1 n + 16 rows, evaluate them in float64, drop the rows with a pre-activation inside its own bound and keep the first n; at most
    5 % of the drawn rows may be dropped (a condition on the inputs, not a tolerance)"""
    m = n + n // 10 + 16
    rows = draw(m)
    safe = safe_of(rows)
    share = 1.0 - float(safe.double().mean())
    print(f"[loss-f64] {name}: ReLU filter dropped {100 * share:.3f} % of {m} drawn rows")
    assert share <= 0.05, f"{name}: {100 * share:.2f} % of the drawn rows dropped"
    keep = torch.nonzero(safe)[:n, 0]
    assert keep.numel() == n
    return [None if t is None else t[keep].contiguous() for t in rows]


def learn_crf(seed, E, scale=1.0):
    from evdeblurnerf_amd import weights as W
    key = ("learn", seed, E, scale)
    if key not in _CRFS:
        sd = {k: (v * (scale if v.ndim == 2 else 1.0)).astype(np.float32) for k, v in W.make_crf_state_dict(seed, E).items()}
        crf = CRF("learn", state_dict=sd, extra_features=E)
        params = LR.pack_params(sd, E)
        assert np.array_equal(crf.flat_params(device="cpu").detach().numpy(), params)      # evd_crf_get_params: the gradient layout
        _CRFS[key] = (crf, params)
    return _CRFS[key]


def test_blur_loss_learn_forward_k_blur_loss():
    """the image branch with live weights (forward only; evd_blur_loss_bwd rejects it)"""
    crf, params = learn_crf(51, 0)
    for i, (R, P) in enumerate([(1, 1), (22, 5), (257, 10), (1024, 16)]):
        pres = PRESENCE[7 - i]
        has0, has2, hast = pres
        pick = lambda t: [t[0], t[1] if has0 else None, t[2], t[3] if has2 else None, t[4], t[5] if hast else None]
        ref = lambda t: LR.blur_loss(t[0], t[2], t[4], rgb0_p=t[1], w2=t[3], tgt0=t[5], map_type="learn", params=params)
        t = draw_safe(f"blur learn R={R} P={P}", R, lambda m: pick(blur_inputs(m, P, 40 + i, False)), lambda t: ref(t)["safe"])
        partial = torch.zeros(8, device=DEV)
        cols = blur_fwd(crf, False, *t, partial, True)
        r = ref(t)
        assert bool(r["safe"].all())
        check(f"k_blur_loss learn R={R} P={P} presence={pres} partial[0:5]", partial[:5], r["partial"][:5], r["E_partial"][:5])
        assert float(partial[5]) == 3 * R
        check(f"k_blur_loss learn R={R} P={P} rgb", cols["rgb"], r["rgb"], r["E_rgb"])


# ---- evd_crf_forward ------------------------------------------------------------------------------------------------------------------
CRF_CASES = [("none", 0), ("gamma", 0), ("learn", 0), ("learn", 1), ("learn", 2), ("learn", 7)]


@pytest.mark.parametrize("kind,E", CRF_CASES, ids=[f"k_crf_forward-{k}-E{e}" for k, e in CRF_CASES])
def test_crf_forward_matches_float64(kind, E):
    crf, params = learn_crf(60 + E, E) if kind == "learn" else (crf_of(kind), None)
    i = 0
    for n in (1, 255, 256, 257):
        for per_ch in ((0, 1) if E else (0,)):
            for luma in (-1, 0, 1, 2):
                for skip in ((False, True) if kind == "learn" else (False,)):
                    def draw(m):
                        g = torch.Generator(device=DEV).manual_seed(1000 * n + 10 * i + E)
                        x = 0.02 + 0.96 * torch.rand((m, 3), generator=g, device=DEV)
                        ft = None
                        if E:
                            ft = torch.randint(-3, 4, (m, 3, E) if per_ch else (m, E), generator=g, device=DEV).float() * (0.5 if E == 7 else 1.0)
                        return [x, ft]
                    name = f"k_crf_forward {kind} E={E} n={n} per_channel={per_ch} luma={luma} skip_learn={int(skip)}"
                    x, ft = draw_safe(name, n, draw, lambda t: LR.crf(t[0], t[1], params, kind, skip, luma)[2]) if kind == "learn" and not skip else draw(n)
                    out = torch.full((n, 3 if luma < 0 else 1), float("nan"), device=DEV)
                    L.check(L.lib().evd_crf_forward(crf.handle, L.ptr(x), L.ptr(ft), per_ch, int(skip), luma, n, L.ptr(out), L.stream_ptr()), "evd_crf_forward")
                    torch.cuda.synchronize()
                    v, Eb, safe = LR.crf(x, ft, params, kind, skip, luma)
                    assert bool(safe.all())
                    check(name, out, v, Eb)
                    i += 1


# ---- evd_event_loss_reduce / evd_event_loss_bwd{,_dev} ----------------------------------------------------------------------------------
EVENT_N = [1, 15, 16, 17, 37, 277, 4097]
EVENT_MODES = {
    "none": dict(kind="none"),
    "gamma": dict(kind="gamma"),
    "gamma-tonemap_only-mask-weights": dict(kind="gamma", tonemap_only=True, mask=True, cw=[0.4, 0.2, 0.4]),
    "none-tonemap_only-no_mask": dict(kind="none", tonemap_only=True),
    "learn-add_bii1": dict(kind="learn", add_bii=1),
    "learn_x3-add_bii1": dict(kind="learn", add_bii=1, scale=3.0),
    "learn-add_bii2-tonemap_only-mask-weights": dict(kind="learn", add_bii=2, tonemap_only=True, mask=True, cw=[0.4, 0.2, 0.4]),
    "learn-add_bii0-tonemap_only-mask": dict(kind="learn", add_bii=0, tonemap_only=True, mask=True),
    "learn-add_bii0-tonemap_only-no_mask": dict(kind="learn", add_bii=0, tonemap_only=True),
    "learn-add_bii1-skip_learn": dict(kind="learn", add_bii=1, skip_learn=True),
}


def event_draw(m, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ev = lambda: (0.05 + 0.9 * torch.rand((m, 3), generator=g, device=DEV)).contiguous()
    es, ee, es0, ee0 = ev(), ev(), ev(), ev()
    cn = -torch.randint(0, 4, (m,), generator=g, device=DEV).float()
    cp = torch.randint(0, 4, (m,), generator=g, device=DEV).float()
    cm = torch.zeros((m, 3), dtype=torch.uint8, device=DEV)
    cm[torch.arange(m, device=DEV), torch.randint(0, 3, (m,), generator=g, device=DEV)] = 1
    return [es, ee, es0, ee0, cn, cp, cm]


def event_call(entry, crf, skip, add_bii, tonemap_only, es, ee, es0, ee0, cn, cp, cm, cw, tail):
    cwa = np.ascontiguousarray(cw, dtype=np.float32) if cw is not None else None
    L.check(getattr(L.lib(), entry)(crf.handle, int(skip), add_bii, int(tonemap_only), L.ptr(es), L.ptr(ee), L.ptr(es0), L.ptr(ee0), L.ptr(cn), L.ptr(cp),
                                    0.2, 0.25, L.ptr(cm), cwa.ctypes.data_as(C.POINTER(C.c_float)) if cwa is not None else None, es.shape[0], *tail,
                                    L.stream_ptr()), entry)
    torch.cuda.synchronize()


def event_case(name, mode, N, pair, dev_entry, want_params, seed):
    mode = dict(mode)
    kind, skip, add_bii, tonemap_only = mode["kind"], mode.get("skip_learn", False), mode.get("add_bii", 0), mode.get("tonemap_only", False)
    crf, params = learn_crf(51, 2, mode.get("scale", 1.0)) if kind == "learn" else (crf_of(kind), None)
    cw = mode.get("cw")
    live = kind == "learn" and not skip
    kw = dict(params=params, map_type=kind, skip_learn=skip, add_bii=add_bii, tonemap_only=tonemap_only, cw=cw)

    def ref_fwd(t):
        return LR.event_loss(t[0], t[1], t[4], t[5], 0.2, 0.25, start0=t[2] if pair else None, end0=t[3] if pair else None,
                             cmask=t[6] if mode.get("mask") else None, **kw)
    t = draw_safe(name, N, lambda m: event_draw(m, seed), lambda t: ref_fwd(t)["safe"]) if live else event_draw(N, seed)
    es, ee, es0, ee0, cn, cp, cm = t
    if not pair:
        es0 = ee0 = None
    if not mode.get("mask"):
        cm = None
    partial = torch.zeros(4, device=DEV)
    event_call("evd_event_loss_reduce", crf, skip, add_bii, tonemap_only, es, ee, es0, ee0, cn, cp, cm, cw, (L.ptr(partial),))
    r = ref_fwd(t)
    assert bool(r["safe"].all())
    check(f"{name} partial[0:3]", partial[:3], r["partial"], r["E_partial"])
    if cw is None:
        assert float(partial[2]) == N, f"{name}: partial[2] = {float(partial[2])}, expected exactly {N}"
    if not pair:
        assert float(partial[1]) == 0.0
    assert float(partial[3]) == 0.0
    g_f, g_c = 0.7, -1.3
    o = dict(d_start=torch.full_like(es, float("nan")), d_end=torch.full_like(es, float("nan")), d_start0=torch.full_like(es, 1234.5),
             d_end0=torch.full_like(es, 1234.5), d_params=torch.full((LR.CRF_NPARAM,), float("nan"), device=DEV))
    outs = (L.ptr(o["d_start"]), L.ptr(o["d_end"]), L.ptr(o["d_start0"]), L.ptr(o["d_end0"]), L.ptr(o["d_params"]) if want_params else None)
    if dev_entry:
        gd = torch.tensor([g_f, g_c], dtype=torch.float32, device=DEV)
        event_call("evd_event_loss_bwd_dev", crf, skip, add_bii, tonemap_only, es, ee, es0, ee0, cn, cp, cm, cw, (L.ptr(gd),) + outs)
    else:
        event_call("evd_event_loss_bwd", crf, skip, add_bii, tonemap_only, es, ee, es0, ee0, cn, cp, cm, cw, (g_f, g_c) + outs)
    rb = LR.event_loss_bwd(t[0], t[1], t[4], t[5], 0.2, 0.25, float(np.float32(g_f)), float(np.float32(g_c)), start0=es0, end0=ee0, cmask=cm, **kw)
    for k in ("d_start", "d_end", "d_start0", "d_end0"):
        if k in rb:
            check(f"{name} {k}", o[k], rb[k], rb["E_" + k])
        else:
            assert (o[k] == 1234.5).all(), f"{name}: {k} written without the coarse pair"
    if want_params:
        if live:
            check(f"{name} d_params", o["d_params"], rb["d_params"], rb["E_d_params"])
            assert (o["d_params"][:128].reshape(16, 8)[:, 3:] == 0).all(), f"{name}: padding columns of the w0 gradient are not exactly 0"
        else:
            assert (o["d_params"] == 0).all(), f"{name}: d_params not zero without a live learn CRF"


@pytest.mark.parametrize("mode", list(EVENT_MODES), ids=[f"k_event_loss+k_event_loss_bwd-{m}" for m in EVENT_MODES])
def test_event_loss_matches_float64(mode):
    i = list(EVENT_MODES).index(mode)
    for j, N in enumerate(EVENT_N):
        for pair in ((True, False) if N in (17, 277) else (bool((i + j) % 2 == 0),)):
            event_case(f"event {mode} N={N} pair={int(pair)}", EVENT_MODES[mode], N, pair, dev_entry=bool((i + j) % 2), want_params=(j % 3 != 1),
                       seed=100 * i + N + int(pair))


def test_event_loss_rejects_bii_features_without_two_extra_inputs():
    """bii features fed to a learn CRF need extra_features == 2, in the forward and in both backward entries"""
    crf, _ = learn_crf(43, 0)
    es, ee, es0, ee0, cn, cp, cm = event_draw(5, 1)
    partial = torch.zeros(4, device=DEV)
    d = [torch.zeros_like(es) for _ in range(4)]
    dp = torch.zeros(LR.CRF_NPARAM, device=DEV)
    outs = tuple(L.ptr(t) for t in d) + (L.ptr(dp),)
    gd = torch.ones(2, device=DEV)
    for add_bii, tm, mask in ((1, False, None), (2, True, cm)):
        with pytest.raises(L.EvdError):
            event_call("evd_event_loss_reduce", crf, False, add_bii, tm, es, ee, es0, ee0, cn, cp, mask, None, (L.ptr(partial),))
        with pytest.raises(L.EvdError):
            event_call("evd_event_loss_bwd", crf, False, add_bii, tm, es, ee, es0, ee0, cn, cp, mask, None, (1.0, 1.0) + outs)
        with pytest.raises(L.EvdError):
            event_call("evd_event_loss_bwd_dev", crf, False, add_bii, tm, es, ee, es0, ee0, cn, cp, mask, None, (L.ptr(gd),) + outs)
    assert (dp == 0).all()
