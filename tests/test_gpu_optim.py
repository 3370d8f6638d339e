"""GPU tests of the optimizer step in the library (evdeblurnerf_amd/optim.py, csrc/kernels_optim.hip): evd_adam_step / evd_grad_norm
against the float64 restatement tests/optim_ref.py, measured in units of the error torch.optim.Adam(foreach=False, fused=False) in
float32 on the CPU -- the reference's own arithmetic -- has against the same restatement; the hand-over to the PDRF levels (mirrors);
the state dict's interchange with torch.optim.Adam; golden G33's trajectory with this optimizer.

Parity bound: device error / torch error <= 2 normwise (a different but equally valid rounding order, FMA contraction for one, can about
double a normwise rounding error; a wrong formula -- a missing bias correction, eps inside the root, decoupled decay -- shows as >= 1e3).
Measured ratios: profiles/optim_parity.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
from evdeblurnerf_amd import _lib as L, optim as O, weights as W
from test_gpu_train_engine import _c2f_model, _rays

pytestmark = pytest.mark.gpu
DEV = "cuda"

# every head / tail combination of the 16-byte body: each length at element offsets 0..3 of a 16-byte-aligned flat buffer; the last length
# spans 513 chunks, so that the 2172 chunks of the table wrap round the capped grid of 2048 workgroups inside the large segments (they come
# last); 80 segments of length 7 in front: 116 segments cannot sit in kernel arguments
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 4097, (1 << 20) + 3]
SEGS = [(7, i % 4) for i in range(80)] + [(n, off) for n in LENGTHS for off in range(4)]
GUARD = 9
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.), dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=2e-4)]
GROUP_OF = [i % 2 for i in range(len(SEGS))]
STEP0 = [(0, 1, 999)[i % 3] for i in range(len(SEGS))]        # differing bias corrections within one call
CLIP = [i % 4 != 3 for i in range(len(SEGS))]
SENTINEL = {"p": -7.25, "g": 3.5, "m": 11.125, "v": -0.625}
STEPS = 5
BOUND = 2.0


def _starts(phases):
    pos, out = 0, []
    for (n, _), ph in zip(SEGS, phases):
        pos += GUARD
        pos += (ph - pos) % 4
        out.append(pos)
        pos += n
    return out, (pos + GUARD + 3) // 4 * 4


P_START, P_TOTAL = _starts([ph for _, ph in SEGS])
# the gradients of every seventh segment (one of the large ones among them) sit at ANOTHER phase than their parameter: the element-wise path
G_START, G_TOTAL = _starts([(ph + 1) % 4 if i % 7 == 3 else ph for i, (_, ph) in enumerate(SEGS)])


def _gradients(rs):
    out = []
    for n, _ in SEGS:
        g = (10.0 ** rs.uniform(-8, 2, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)
        g[16::17] = 0.0                                         # exact zeros
        g[5::19] = np.float32(1e-40)                            # float32 subnormals
        g[11::19] = np.float32(-3e-42)
        out.append(g)
    return out


class Case:
    """inputs (float32 numpy), shared by every test of the kernels; never modified"""

    def __init__(self):
        rs = np.random.RandomState(2024)
        self.p0 = [rs.normal(0, 0.1, n).astype(np.float32) for n, _ in SEGS]
        self.m0 = [(rs.normal(0, 1e-2, n) if s else np.zeros(n)).astype(np.float32) for (n, _), s in zip(SEGS, STEP0)]
        self.v0 = [(rs.uniform(0, 1e-3, n) if s else np.zeros(n)).astype(np.float32) for (n, _), s in zip(SEGS, STEP0)]
        self.grads = [_gradients(rs) for _ in range(STEPS)]


def cat64(arrs):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in arrs])


def run_ref64(case, grads_per_step, max_norm=None, coef=None):
    """-> [(params, exp_avg, exp_avg_sq) concatenated, after every step] of the float64 restatement"""
    ref = R.Adam(case.p0, GROUP_OF, GROUPS)
    ref.step_count = list(STEP0)
    ref.exp_avg, ref.exp_avg_sq = [a.astype(np.float64) for a in case.m0], [a.astype(np.float64) for a in case.v0]
    out = []
    for grads in grads_per_step:
        ref.step(grads, max_norm=max_norm, clip=CLIP, coef=coef)
        out.append((cat64(ref.params), cat64(ref.exp_avg), cat64(ref.exp_avg_sq)))
    return out


def run_torch32(case, grads_per_step, max_norm=None, norms=None):
    """the same with torch.optim.Adam(foreach=False, fused=False) (+ clip_grad_norm_) in float32 on the CPU; norms: a list that
    receives clip_grad_norm_'s float32 total norms"""
    ps = [torch.tensor(p, requires_grad=True) for p in case.p0]
    opt = torch.optim.Adam([dict(params=[p for p, k in zip(ps, GROUP_OF) if k == j], **GROUPS[j]) for j in range(2)], foreach=False, fused=False)
    for p, m, v, s in zip(ps, case.m0, case.v0, STEP0):
        opt.state[p] = {"step": torch.tensor(float(s)), "exp_avg": torch.tensor(m), "exp_avg_sq": torch.tensor(v)}
    out = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.tensor(g)
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_([p for p, c in zip(ps, CLIP) if c], max_norm, foreach=False)
            if norms is not None:
                norms.append(tn)
        opt.step()
        out.append((cat64([p.detach().numpy() for p in ps]), cat64([opt.state[p]["exp_avg"].numpy() for p in ps]),
                    cat64([opt.state[p]["exp_avg_sq"].numpy() for p in ps])))
    return out


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module")
def five_steps(case):
    return run_ref64(case, case.grads), run_torch32(case, case.grads)


class Device:
    """the case on the device: four flat buffers with guard elements between and around all segments, and the segment table over them"""

    def __init__(self, case, mirrors=False):
        def flat(total, starts, arrs, fill):
            t = torch.full((total,), fill, dtype=torch.float32, device=DEV)
            mask = torch.ones((total,), dtype=torch.bool, device=DEV)
            for s, a in zip(starts, arrs):
                t[s:s + len(a)] = torch.as_tensor(a, device=DEV)
                mask[s:s + len(a)] = False
            return t, mask
        self.p, self.pmask = flat(P_TOTAL, P_START, case.p0, SENTINEL["p"])
        self.m, _ = flat(P_TOTAL, P_START, case.m0, SENTINEL["m"])
        self.v, _ = flat(P_TOTAL, P_START, case.v0, SENTINEL["v"])
        self.g, self.gmask = flat(G_TOTAL, G_START, case.grads[0], SENTINEL["g"])
        self.f32 = torch.full((P_TOTAL,), SENTINEL["p"], dtype=torch.float32, device=DEV) if mirrors else None
        self.f16 = torch.full((P_TOTAL,), SENTINEL["p"], dtype=torch.float16, device=DEV) if mirrors else None
        at = lambda t, s, b=4: t.data_ptr() + b * s
        rows = [(at(self.p, s), at(self.m, s), at(self.v, s), at(self.f32, s) if mirrors else None, at(self.f16, s, 2) if mirrors else None, n, k, c)
                for s, (n, _), k, c in zip(P_START, SEGS, GROUP_OF, CLIP)]
        self.seg = O._Segments(rows, 2, DEV)
        self.steps = (C.c_long * len(SEGS))(*STEP0)
        self.groups = (L.AdamGroup * 2)()
        for gc, g in zip(self.groups, GROUPS):
            gc.lr, (gc.beta1, gc.beta2), gc.eps, gc.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        self.set_grads(case.grads[0])

    def set_grads(self, grads):
        for i, (s, a) in enumerate(zip(G_START, grads)):
            if a is None:
                self.seg.grads[i] = None
            else:
                self.g[s:s + len(a)] = torch.as_tensor(a, device=DEV)
                self.seg.grads[i] = self.g.data_ptr() + 4 * s

    def step(self, max_norm=None, zero_grads=False):
        if max_norm is not None:
            self.seg.grad_norm()
        L.check(L.lib().evd_adam_step(self.seg._h, self.seg.grads, self.steps, self.groups, 2, float(max_norm or 0.), L.ptr(self.seg.norm) if max_norm else None,
                                      int(zero_grads), L.ptr(self.seg.ws), self.seg.nbytes, L.stream_ptr()), "evd_adam_step")
        for i in range(len(SEGS)):
            self.steps[i] += self.seg.grads[i] is not None

    def guards_intact(self):
        ok = lambda t, mask, fill: bool((t[mask] == fill).all())
        return (ok(self.p, self.pmask, SENTINEL["p"]) and ok(self.m, self.pmask, SENTINEL["m"]) and ok(self.v, self.pmask, SENTINEL["v"])
                and ok(self.g, self.gmask, SENTINEL["g"]) and (self.f32 is None or (ok(self.f32, self.pmask, SENTINEL["p"]) and ok(self.f16, self.pmask, SENTINEL["p"]))))

    def get(self):
        cut = lambda t: cat64([t[s:s + n].cpu().numpy() for s, (n, _) in zip(P_START, SEGS)])
        return cut(self.p), cut(self.m), cut(self.v)


def ratios(dev, ref, tch, p0):
    """normwise error of the device / of torch's float32 against the restatement, for the parameter change and both moments"""
    out = {}
    for name, d, r, t in zip(("param change", "exp_avg", "exp_avg_sq"), dev, ref, tch):
        if name == "param change":
            d, r, t = d - p0, r - p0, t - p0
        e_dev, e_t = np.linalg.norm(d - r), np.linalg.norm(t - r)
        assert e_t > 0 and np.isfinite(e_dev)
        out[name] = (e_dev / e_t, e_dev / np.linalg.norm(r), e_t / np.linalg.norm(r))
    return out


def show(tag, rt):
    for k, (ratio, e_dev, e_t) in rt.items():
        print(f"optim parity [{tag}] {k}: device / torch = {ratio:.3f}   (device {e_dev:.2e}, torch float32 {e_t:.2e} of the norm)")


def test_five_steps_against_the_float64_restatement(case, five_steps):
    ref, tch = five_steps
    d = Device(case, mirrors=True)
    p0 = cat64(case.p0)
    g_before = d.g.clone()
    for s in range(STEPS):
        if s:
            d.set_grads(case.grads[s])
            g_before = d.g.clone()
        d.step()
        assert d.guards_intact(), s
        assert torch.equal(d.g.view(torch.int32), g_before.view(torch.int32))          # the gradients are read, not written
        if s in (0, STEPS - 1):
            rt = ratios(d.get(), ref[s], tch[s], p0)
            show(f"{s + 1} step{'s' * (s > 0)}", rt)
            assert max(v[0] for v in rt.values()) <= BOUND, rt
    # the mirrors hold the parameters: float32 bit for bit, float16 by the saturating conversion of the grid loader (exercised on these values
    # below 65504 as round-to-nearest; the saturation itself is pinned by the f16 render of test_mirrors_*)
    inside = ~d.pmask
    assert torch.equal(d.f32[inside].view(torch.int32), d.p[inside].view(torch.int32))
    assert torch.equal(d.f16[inside].view(torch.int16), d.p[inside].half().view(torch.int16))
    assert [d.steps[i] for i in range(len(SEGS))] == [s + STEPS for s in STEP0]


def test_float16_mirror_saturates_like_the_grid_loader():
    """values beyond the float16 range: +-65504, not inf (f16_sat); NaN stays NaN"""
    vals = torch.tensor([1e5, -1e5, 65504.0, 65520.0, 7e4, -3e38, 1.0, float("nan"), 65519.0], device=DEV)
    p, m, v, g = vals.clone(), torch.zeros_like(vals), torch.zeros_like(vals), torch.zeros_like(vals)
    f16 = torch.zeros((len(vals),), dtype=torch.float16, device=DEV)
    seg = O._Segments([(p.data_ptr(), m.data_ptr(), v.data_ptr(), None, f16.data_ptr(), len(vals), 0, 0)], 1, DEV)
    seg.grads[0] = g.data_ptr()
    groups = (L.AdamGroup * 1)()
    groups[0].lr, groups[0].beta1, groups[0].beta2, groups[0].eps, groups[0].weight_decay = 1e-3, 0.9, 0.999, 1e-8, 0.
    L.check(L.lib().evd_adam_step(seg._h, seg.grads, (C.c_long * 1)(0), groups, 1, 0., None, 0, L.ptr(seg.ws), seg.nbytes, L.stream_ptr()), "evd_adam_step")
    ok = ~vals.isnan()
    assert torch.equal(p[ok].view(torch.int32), vals[ok].view(torch.int32)) and bool(p[7].isnan())      # a zero gradient moves nothing
    want = vals.clamp(-65504.0, 65504.0).half()
    assert torch.equal(f16[~want.isnan()], want[~want.isnan()]) and bool(f16[7].isnan()) and not bool(f16.isinf().any())


def test_grad_norm_is_the_rounded_float64_norm_and_reproducible(case):
    d = Device(case)
    want = np.float32(R.total_norm([g for g, c in zip(case.grads[0], CLIP) if c]))
    a = d.seg.grad_norm().clone()
    b = d.seg.grad_norm().clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    print(f"evd_grad_norm {float(a):.9g}, float64 norm rounded {float(want):.9g}")
    assert abs(np.float32(a.item()) - want) <= np.spacing(want)
    skipped = list(case.grads[0])
    skipped[113] = skipped[2] = None                            # a flagged large segment and a small one without gradient: left out
    assert CLIP[113] and CLIP[2]
    d.set_grads(skipped)
    want = np.float32(R.total_norm([g for g, c in zip(skipped, CLIP) if c and g is not None]))
    assert abs(np.float32(d.seg.grad_norm().item()) - want) <= np.spacing(want)
    assert d.guards_intact()


def coef32(norm, max_norm):
    """clip_grad_norm_'s coefficient as float32 arithmetic forms it from a float32 norm: clamp(max_norm / (norm + 1e-6), max=1), the
    division of a number by a tensor being reciprocal times number"""
    c = np.float32(1) / (np.float32(norm) + np.float32(1e-6)) * np.float32(max_norm)
    return float(min(c, np.float32(1)))


@pytest.mark.parametrize("frac", [0.1, 10.0, None])
def test_clip_inside_the_step(case, frac):
    """A clip that bites (max_norm = a tenth of the norm), one that does not, and none; the stored gradients are not rewritten.
    The bound: the coefficient is a float32 scalar formed in four rounded operations (norm, + 1e-6, reciprocal, product), so it carries up
    to 4 x 2^-24 of relative error into EVERY clipped gradient at once -- on the device as in torch, each from its own float32 norm.
    That common factor is not rounding noise of the element arithmetic and is pinned separately: the device norm is the rounded float64
    norm to 1 ulp (test_grad_norm_*), and the coefficient the device used is coef32 of that norm -- the restatement is run with exactly
    this number, so another formula on the device would miss by far more than rounding.  The element arithmetic then holds the parity
    bound against torch's float32 run measured the same way (against the restatement run with torch's own coefficient)."""
    max_norm = None if frac is None else frac * R.total_norm([g for g, c in zip(case.grads[0], CLIP) if c])
    d = Device(case)
    g_before = d.g.clone()
    d.step(max_norm=max_norm)
    assert d.guards_intact() and torch.equal(d.g.view(torch.int32), g_before.view(torch.int32))
    norms = []
    tch = run_torch32(case, case.grads[:1], max_norm, norms)[0]
    ref_t = ref_d = run_ref64(case, case.grads[:1])[0]
    if frac is not None:
        c_d, c_t = coef32(d.seg.norm.item(), max_norm), coef32(norms[0].item(), max_norm)
        exact = R.clip_coef(R.total_norm([g for g, c in zip(case.grads[0], CLIP) if c]), max_norm)
        print(f"clip coefficient: device {c_d:.9g}, torch {c_t:.9g}, float64 {exact:.9g}")
        assert abs(c_d - exact) <= 4 * 2.0 ** -24 * exact and (c_d == 1.0) == (frac > 1)
        ref_d, ref_t = run_ref64(case, case.grads[:1], max_norm, c_d)[0], run_ref64(case, case.grads[:1], max_norm, c_t)[0]
    p0 = cat64(case.p0)
    rt = {}
    for k, (name, dv, tv) in enumerate(zip(("param change", "exp_avg", "exp_avg_sq"), d.get(), tch)):
        e_dev, e_t = np.linalg.norm(dv - ref_d[k]), np.linalg.norm(tv - ref_t[k])
        scale = np.linalg.norm(ref_d[k] - (p0 if k == 0 else 0))
        rt[name] = (e_dev / e_t, e_dev / scale, e_t / scale)
    show(f"clip {frac}", rt)
    assert max(v[0] for v in rt.values()) <= BOUND, rt
    if frac == 0.1:                                             # the clip did bite: the unclipped step is far away
        unclipped = run_ref64(case, case.grads[:1])[0]
        assert np.linalg.norm(unclipped[1] - ref_d[1]) > 0.5 * np.linalg.norm(ref_d[1])


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_non_finite_gradients_propagate_as_in_torch(case, max_norm):
    grads = [g.copy() for g in case.grads[0]]
    grads[100][7] = np.inf                                      # two flagged segments
    grads[108][200] = np.nan
    assert CLIP[100] and CLIP[108]
    tch = run_torch32(case, [grads], max_norm)[0]
    d = Device(case)
    d.set_grads(grads)
    d.step(max_norm=max_norm)
    if max_norm is not None:
        assert bool(d.seg.norm.isnan().all())
    assert d.guards_intact()
    for got, want in zip(d.get(), tch):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.isnan(d.get()[0]).sum() >= (2 if max_norm is None else sum(n for (n, _), c in zip(SEGS, CLIP) if c))


# ------------------------------------------------------------------------------------------------ optim.Adam on the same buffers
def _leaves(d):
    ps = [d.p[s:s + n].detach().requires_grad_(True) for s, (n, _) in zip(P_START, SEGS)]
    groups = [dict(params=[p for p, k in zip(ps, GROUP_OF) if k == j], **GROUPS[j]) for j in range(2)]
    order = [i for j in range(2) for i, k in enumerate(GROUP_OF) if k == j]         # the optimizer's parameter order
    return ps, groups, order


def test_skipped_parameters_and_zero_grads(case):
    d = Device(case)
    ps, groups, order = _leaves(d)
    opt = O.Adam(groups, zero_grads=True)
    gviews = [d.g[s:s + n] for s, (n, _) in zip(G_START, SEGS)]
    for p, g in zip(ps, gviews):
        p.grad = g
    opt.step()                                                  # every parameter has state now
    assert all(bool((g == 0).all()) for g in gviews) and all(p.grad is g for p, g in zip(ps, gviews))
    assert bool((d.g[d.gmask] == SENTINEL["g"]).all()) and bool((d.p[d.pmask] == SENTINEL["p"]).all())
    snap = lambda: [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"])) for p in ps]
    before = snap()
    none = {3, 50, 81, 115}                                     # small ones and the last large one
    d.set_grads(case.grads[1])
    for i, p in enumerate(ps):
        if i in none:
            p.grad = None
    opt.step()
    after = snap()
    for i, (b, a) in enumerate(zip(before, after)):
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b[:3], a[:3]))
        assert same == (i in none) and a[3] == b[3] + (i not in none), i
        assert ps[i].grad is None if i in none else (ps[i].grad is gviews[i] and bool((gviews[i] == 0).all()))
    opt.zero_grad(set_to_none=False)                            # stays correct after the fused clearing
    assert all(p.grad is None or bool((p.grad == 0).all()) for p in ps)
    sd = opt.state_dict()
    assert [float(sd["state"][k]["step"]) for k in range(len(ps))] == [2. - (order[k] in none) for k in range(len(ps))]


def test_no_host_device_traffic_in_a_loop_of_steps(case):
    """what tools/trace_h2d.py watches for -- an aten op whose tensors are not all on one device, a synchronising pageable copy each --
    over a loop of steps with clipping: nothing"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if len({t.device.type for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)}) > 1:
                seen.append(str(func))
            return out

    d = Device(case)
    ps, groups, _ = _leaves(d)
    opt = O.Adam(groups, max_grad_norm=1.0, zero_grads=True)
    for p, s, (n, _) in zip(ps, G_START, SEGS):
        p.grad = d.g[s:s + n]
    opt.step()                                                  # builds the table (one-off uploads)
    with Watch():
        for _ in range(4):
            for g in opt.param_groups:
                g["lr"] = g["lr"] * 0.9
            opt.step()
    assert seen == []
    assert opt.total_norm is not None and float(opt.total_norm) == 0.0          # (the gradients were cleared by the first step)


def test_stand_alone_clip_grad_norm(case):
    d = Device(case)
    ps, _, _ = _leaves(d)
    for p, s, (n, _) in zip(ps, G_START, SEGS):
        p.grad = d.g[s:s + n]
    want = R.total_norm(case.grads[0])
    total = O.clip_grad_norm_(ps, 0.1 * want)
    assert total.is_cuda and abs(np.float32(total.item()) - np.float32(want)) <= np.spacing(np.float32(want))
    got = cat64([p.grad.cpu().numpy() for p in ps])
    assert np.linalg.norm(got - 0.1 * cat64(case.grads[0])) <= 1e-6 * 0.1 * want
    assert bool((d.g[d.gmask] == SENTINEL["g"]).all())


# ------------------------------------------------------------------------------------------------ interchange with torch.optim.Adam
def _small(seed=3):
    rs = np.random.RandomState(seed)
    shapes = [(33, 7), (5,), (1025,), (2, 3, 4)]
    p0 = [rs.normal(0, 0.1, sh).astype(np.float32) for sh in shapes]
    grads = [[(rs.normal(0, 1, sh) * 10.0 ** rs.uniform(-3, 1)).astype(np.float32) for sh in shapes] for _ in range(4)]
    return p0, grads


def _groups(ps):
    return [dict(params=ps[:2], **GROUPS[0], initial_lr=1e-3), dict(params=ps[2:], **GROUPS[1], initial_lr=5e-4)]


@pytest.mark.parametrize("first", ["torch", "library"])
def test_state_dict_interchanges_with_torch_adam(first):
    p0, grads = _small()
    ref = R.Adam(p0, [0, 0, 1, 1], GROUPS)
    cpu = [torch.tensor(p, requires_grad=True) for p in p0]
    copt = torch.optim.Adam(_groups(cpu), foreach=False, fused=False)
    for gs in grads:
        ref.step(gs)
        for p, g in zip(cpu, gs):
            p.grad = torch.tensor(g)
        copt.step()
    ps = [torch.tensor(p, device=DEV, requires_grad=True) for p in p0]
    make = {"torch": lambda: torch.optim.Adam(_groups(ps), foreach=False), "library": lambda: O.Adam(_groups(ps))}
    a, b = make[first](), make["library" if first == "torch" else "torch"]()

    def two(opt, gss):
        for gs in gss:
            for p, g in zip(ps, gs):
                p.grad = torch.tensor(g, device=DEV)
            opt.step()

    two(a, grads[:2])
    sd = a.state_dict()
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) == 2
               for st, p in zip((sd["state"][k] for k in range(4)), ps))
    assert all(g["initial_lr"] in (1e-3, 5e-4) and {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"} <= set(g) for g in sd["param_groups"])
    b.load_state_dict(sd)
    two(b, grads[2:])
    assert all(float(b.state[p]["step"]) == 4 for p in ps)
    p0c = cat64(p0)
    mixed = (cat64([p.detach().cpu().numpy() for p in ps]), cat64([b.state[p]["exp_avg"].cpu().numpy() for p in ps]),
             cat64([b.state[p]["exp_avg_sq"].cpu().numpy() for p in ps]))
    tch = (cat64([p.detach().numpy() for p in cpu]), cat64([copt.state[p]["exp_avg"].numpy() for p in cpu]), cat64([copt.state[p]["exp_avg_sq"].numpy() for p in cpu]))
    rt = ratios(mixed, (cat64(ref.params), cat64(ref.exp_avg), cat64(ref.exp_avg_sq)), tch, p0c)
    show(f"2 {first} steps, state dict, 2 steps of the other", rt)
    assert max(v[0] for v in rt.values()) <= BOUND, rt


# ------------------------------------------------------------------------------------------------ the hand-over to the library
KW = dict(ndc=True, near=0., far=1., use_viewdirs=True, N_samples=24, N_importance=16, raw_noise_std=0., perturb=0.)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _load_grids_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ka = prof.key_averages()
    assert sum(e.count for e in ka if e.device_time_total > 0) > 0              # the profiler saw the device
    return sum(e.count for e in ka if "k_load_grids" in e.key)


def test_mirrors_hand_the_grids_to_the_levels():
    """Two identical models, one backward of the same loss each.  A steps with optim.Adam(model=A): its levels' float32 copies equal its
    leaves bit for bit, an f16 render (which gathers the float16 copies) equals that of B -- which received the same update and an
    explicit load_grids -- bit for bit, and A's next forward launches no k_load_grids."""
    K = W.synthetic_camera()
    rays = _rays(256, 9, requires_grad=False)
    tgt = torch.rand((256, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    models = []
    for _ in range(2):
        model, sd = _c2f_model("f16x3", 16)
        model.enable_training(sd, grads_in_place=True).train()
        rgb, rgb0, other, _ = model(400, 400, K, 1 << 22, rays=rays, **KW)
        (((rgb - tgt) ** 2).mean() + ((rgb0 - tgt) ** 2).mean() + 1e-3 * other["TV"].sum()).backward()
        models.append(model)
    A, B = models
    grads = [p.grad for p in A.parameters()]
    assert all(g is not None for g in grads)
    opt = O.Adam(A.parameters(), lr=2e-3, model=A, zero_grads=True)
    before = [p.detach().clone() for p in A.parameters()]
    opt.step()
    assert all(p.grad is g and bool((g == 0).all()) for p, g in zip(A.parameters(), grads))
    assert all(float((p.detach() - q).abs().max()) > 0 for p, q in zip(A.parameters(), before))
    with torch.no_grad():
        for pa, pb in zip(A.parameters(), B.parameters()):
            pb.copy_(pa)
    B.invalidate_packed()
    for lv in B._levels:
        lv.net.load_grids(list(lv.grids.values()))
    for lv in A._levels:
        for leaf, kept in zip(lv.grids.values(), lv.net.grid_params()):                 # evd_voxel_get_grids
            assert _bits_equal(leaf.detach(), kept.detach())

    def f16_render(model):
        model.eval()
        prev, model.precision = model.precision, "f16"
        try:
            return model.render(400, 400, K, rays=rays, ndc=True, near=0., far=1., use_viewdirs=True, N_samples=24, N_importance=16)[0]
        finally:
            model.precision = prev
            model.train()

    ra, rb = f16_render(A), f16_render(B)
    assert bool(torch.isfinite(ra).all()) and _bits_equal(ra, rb)
    pts = torch.rand((64, 8, 3), device=DEV) * 2 - 1
    for la, lb in zip(A._levels, B._levels):
        assert _bits_equal(la.net.sample(pts, "f16"), lb.net.sample(pts, "f16"))
    fwd = lambda m: (lambda: m(400, 400, K, 1 << 22, rays=rays, **KW))
    assert _load_grids_launches(fwd(A)) == 0
    B.invalidate_packed()
    assert _load_grids_launches(fwd(B)) == 2                                           # the control: both levels reload, and the profiler sees it


_TORCH_RUN = {}


@pytest.mark.parametrize("with_model", [True, False])
@pytest.mark.parametrize("in_place", [True, False])
def test_optim_adam_reaches_the_library(in_place, with_model):
    """test_fused_adam_reaches_the_library's scenario with optim.Adam, which writes the parameters through raw pointers (no version counter
    moves): three steps move the render, and it agrees with the torch.optim.Adam(fused=False) run"""
    K = W.synthetic_camera()
    rays = _rays(256, 9, requires_grad=False)
    tgt = torch.rand((256, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))

    def run(make):
        model, sd = _c2f_model("f16x3", 16)
        model.enable_training(sd, grads_in_place=in_place).train()
        opt = make(model)
        first = None
        for _ in range(3):
            rgb, rgb0, _, _ = model(400, 400, K, 1 << 22, rays=rays, tv=False, **KW)
            first = rgb.detach().clone() if first is None else first
            loss = ((rgb - tgt) ** 2).mean() + ((rgb0 - tgt) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        rgb = model(400, 400, K, 1 << 22, rays=rays, tv=False, **KW)[0].detach()
        assert (rgb - first).abs().max() > 1e-3                     # three steps moved the render
        return rgb

    if in_place not in _TORCH_RUN:
        _TORCH_RUN[in_place] = run(lambda m: torch.optim.Adam(m.parameters(), lr=2e-3, fused=False))
    got = run(lambda m: O.Adam(m.parameters(), lr=2e-3, model=m if with_model else None))
    assert (got - _TORCH_RUN[in_place]).abs().max() < 2e-4, float((got - _TORCH_RUN[in_place]).abs().max())


def test_zero_grads_needs_the_in_place_buffers():
    model, sd = _c2f_model("f16x3", 16)
    model.enable_training(sd, grads_in_place=False).train()
    with pytest.raises(L.EvdError):
        O.Adam(model.parameters(), lr=1e-3, model=model, zero_grads=True)


# ------------------------------------------------------------------------------------------------ golden G33 with this optimizer
def test_G33_trajectory_with_the_library_optimizer():
    """test_G33_five_iterations_follow_the_reference_trajectory, case ("f16x3", "fused", True) under that case's bounds, with optim.Adam
    (model given, zero_grads: no optimizer.zero_grad() in the loop) in place of torch's and lr_at in place of the inline decay"""
    from test_gpu_train_call import CALL_KW, G33_CASES, ReplayKernel, _model, _ref_layout
    from conftest import load_golden, maxabs
    from torch_restatement import grad_summary
    from evdeblurnerf_amd.losses import (blur_loss_partials_autograd, crf_param_grads, event_loss_from_partials, event_loss_partials_autograd)
    from evdeblurnerf_amd.tonemapping import CRF
    prec, awp_kind, in_place = "f16x3", "fused", True
    tol = G33_CASES[(prec, awp_kind, in_place)]
    g = load_golden("G33_train_trajectory")
    lrate, lrate_decay, flw, w_pts0, w_egm, w_tv, thr = (float(v) for v in g["scalars"])
    n_steps = len(g["losses"])
    kern = ReplayKernel(g, prefix="s{}.")
    model, awp, sd = _model(33, g, prec, awp_kind, kern, grads_in_place=in_place)
    csd = W.make_crf_state_dict(331, extra_features=2)
    csd = {k: (v * np.float32(3.0) if np.asarray(v).ndim == 2 else v) for k, v in csd.items()}
    crf_rgb, crf_ev = CRF("gamma"), CRF("learn", state_dict=csd, extra_features=2)
    crf_flat = crf_ev.flat_params("cuda")
    groups = [{"params": model.grad_vars, "lr": lrate}, {"params": model.grad_vars_vol, "lr": lrate}, {"params": [crf_flat], "lr": lrate}]
    for gr in groups:
        gr.setdefault("initial_lr", gr["lr"])
    opt = O.Adam(groups, lr=lrate, betas=(0.9, 0.999), model=model, zero_grads=True)
    K = W.synthetic_camera()
    T = lambda k: torch.tensor(g[k], device=DEV)
    rays, ev_start, ev_end, target, target_pts0, cn, cp = (T(k) for k in ("rays", "ev_start", "ev_end", "target", "target_pts0", "cn", "cp"))
    info = {"images_idx": T("images_idx")}
    ones = torch.ones((rays.shape[0], 1), device=DEV)

    def tracked():
        out = {k: _ref_layout(k, v.detach()) for k, v in model.named_parameters() if k.startswith(("mlp_coarse.", "mlp_fine."))}
        out.update({"awp." + k: v.detach() for k, v in awp.named_parameters() if not k.startswith("MAM.conv.")})
        out.update({"crf." + k: v for k, v in crf_param_grads(crf_flat.detach(), 2).items()})
        return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}

    p0 = tracked()
    keys = [k[len("s0.d."):-8] for k in g if k.startswith("s0.d.") and k.endswith(".summary")]
    assert set(keys) == set(p0), set(keys) ^ set(p0)
    global_step, losses, report = 0, [], {}
    for i in range(n_steps):
        kern.step = i
        rgb, rgb0, other, tens = model(400, 400, K, 1 << 20, rays=rays, rays_info=info, force_naive=False, return_pts0_rgb=True, **CALL_KW)
        pa = blur_loss_partials_autograd(crf_rgb, rgb[:, None], ones, target, rgb0_p=rgb0[:, None])
        pb = blur_loss_partials_autograd(crf_rgb, tens["rgb_awp"][:, None], ones, target)
        pc = blur_loss_partials_autograd(crf_rgb, tens["stage1_rgb_pts0"][:, None], ones, target_pts0, rgb0_p=tens["stage1_rgb1_pts0"][:, None])
        n = pa.detach()[5]
        loss = (pa[0] + pa[1]) / n * (1 - flw) + pb[0] / n * flw + (pc[0] + pc[1]) / n * w_pts0
        loss = loss + other["TV"].mean() * w_tv
        s, s0, _, _ = model(400, 400, K, 1 << 20, rays=ev_start, rays_info=None, force_naive=True, **CALL_KW)
        e, e0, _, _ = model(400, 400, K, 1 << 20, rays=ev_end, rays_info=None, force_naive=True, **CALL_KW)
        pe = event_loss_partials_autograd(crf_ev, crf_flat, s, e, cn, cp, thr, thr, start0=s0, end0=e0, add_bii="pos-neg")
        loss = loss + event_loss_from_partials(pe) * w_egm
        loss.backward()                                     # (the gradients were cleared by the previous step)
        opt.step()
        crf_ev.load_params(crf_flat)
        for gr in opt.param_groups:
            gr["lr"] = O.lr_at(gr["initial_lr"], global_step, lrate_decay)
        global_step += 1
        losses.append(float(loss.detach()))
        now = tracked()
        worst = {}
        for idx, key in enumerate(keys):
            if key == "awp.MAM.linear.bias":
                continue
            sm, _ = grad_summary(now[key] - p0[key], 7000 + idx)
            ref = g[f"s{i}.d.{key}.summary"]
            worst[key] = max(abs(sm[0] - ref[0]), abs(sm[1] - ref[1])) / max(float(ref[0]), 1e-30)
        report[i] = worst
    top = lambda d: {k: f"{v:.1e}" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:4]}
    lerr = np.abs(np.array(losses) - g["losses"])
    print("G33 with optim.Adam: losses", [f"{v:.6f}" for v in losses], "reference", [f"{v:.6f}" for v in g["losses"]], f"max diff {lerr.max():.1e}")
    last = tracked()
    value = {}
    for key in keys:
        if f"s{n_steps - 1}.p.{key}" in g and key != "awp.MAM.linear.bias":
            ref = g[f"s{n_steps - 1}.p.{key}"].astype(np.float64)
            value[key] = float(np.linalg.norm(last[key].reshape(ref.shape) - ref) / max(np.linalg.norm(ref), 1e-30))
    lv = {k: v for k, v in report[n_steps - 1].items() if k.startswith("mlp_")}
    sd_ = {k: v for k, v in report[n_steps - 1].items() if not k.startswith("mlp_")}
    print(f"  after step {n_steps - 1}: level change worst {top(lv)}; AWP / CRF worst {top(sd_)}; values worst {top(value)}")
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert lerr.max() < tol["loss"], lerr
    assert max(lv.values()) < tol["level"], top(lv)
    assert max(sd_.values()) < tol["side"], top(sd_)
    assert max(value.values()) < tol["value"], top(value)
    bn = awp.MAM.Corr.convd[1]
    assert int(bn.num_batches_tracked) == int(g["awp.after.num_batches_tracked"]) == n_steps
    assert maxabs(bn.running_mean.cpu().numpy(), g["awp.after.running_mean"]) < 5e-3
