"""CPU-only: the float64 restatement tests/optim_ref.py against torch itself in float64 -- torch.optim.Adam(foreach=False, fused=False),
torch.nn.utils.clip_grad_norm_ -- and evdeblurnerf_amd.optim.lr_at against the schedule of run_nerf.py:603-613.  Both sides evaluate the
same formulas in float64, so they agree to 1e-12 of the norm."""
import numpy as np
import pytest
import torch

import optim_ref as R

SHAPES = [(7, 5), (33,), (4, 3, 2), (1,)]
GROUP_OF = [0, 1, 0, 1]
GROUPS = [dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.), dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=2e-4)]
STEPS = 5
LATE = 2            # parameter 2 has no gradient in steps 0 and 1


def _data(seed=5):
    rs = np.random.RandomState(seed)
    params = [rs.normal(0, 0.1, sh) for sh in SHAPES]
    grads = [[rs.normal(0, 1, sh) * 10.0 ** rs.uniform(-4, 1) for sh in SHAPES] for _ in range(STEPS)]
    for s in range(2):
        grads[s][LATE] = None
    return params, grads


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a).ravel() - np.asarray(b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-300))


@pytest.mark.parametrize("max_norm_frac", [None, 0.1, 10.0])
def test_restatement_matches_torch_adam_and_clip_in_float64(max_norm_frac):
    params, grads = _data()
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    opt = torch.optim.Adam([dict(params=[tp[i] for i in range(4) if GROUP_OF[i] == k], **GROUPS[k]) for k in range(2)], foreach=False, fused=False)
    ref = R.Adam(params, GROUP_OF, GROUPS)
    for s in range(STEPS):
        for p, g in zip(tp, grads[s]):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        max_norm = None
        if max_norm_frac is not None:
            max_norm = max_norm_frac * R.total_norm(grads[s])
            tn = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
        opt.step()
        norm = ref.step(grads[s], max_norm=max_norm)
        if max_norm is not None:
            assert abs(norm - float(tn)) <= 1e-12 * float(tn)
            coef = R.clip_coef(norm, max_norm)
            assert (coef == 1.0) == (max_norm_frac > 1)
            for p, g in zip(tp, grads[s]):
                if g is not None:
                    assert rel(g * coef, p.grad.numpy()) < 1e-12
        for i, p in enumerate(tp):
            assert rel(ref.params[i], p.detach().numpy()) < 1e-12, (s, i)
            if s < 2 and i == LATE:         # no gradient yet: untouched, no state
                assert np.array_equal(ref.params[i], params[i]) and len(opt.state[p]) == 0 and ref.step_count[i] == 0
                continue
            st = opt.state[p]
            assert float(st["step"]) == ref.step_count[i] == (s + 1 - (2 if i == LATE else 0))
            assert rel(ref.exp_avg[i], st["exp_avg"].numpy()) < 1e-12 and rel(ref.exp_avg_sq[i], st["exp_avg_sq"].numpy()) < 1e-12, (s, i)


def test_non_finite_norm_gives_torchs_coefficient():
    for bad in (float("inf"), float("nan")):
        g = torch.tensor([1.0, bad, 2.0], dtype=torch.float64)
        p = torch.zeros(3, dtype=torch.float64, requires_grad=True)
        p.grad = g.clone()
        tn = torch.nn.utils.clip_grad_norm_([p], 1.0, foreach=False)
        norm = R.total_norm([g.numpy()])
        assert np.isnan(norm) == bool(torch.isnan(tn)) and np.isinf(norm) == bool(torch.isinf(tn))
        got = g.numpy() * R.clip_coef(norm, 1.0)
        assert np.array_equal(np.isnan(got), torch.isnan(p.grad).numpy())
        assert np.array_equal(got[~np.isnan(got)], p.grad.numpy()[~np.isnan(got)])


@pytest.mark.parametrize("which", ["package", "restatement"])
def test_lr_at_is_the_reference_schedule(which):
    from evdeblurnerf_amd.optim import lr_at as pkg
    f = pkg if which == "package" else R.lr_at
    lr0, decay, wi, wf = 5e-4, 250, 2000, 0.1

    def expected(step, warmup_iters):       # run_nerf.py:603-613 written out
        if warmup_iters > 0 and step < warmup_iters:
            return lr0 * ((1 - wf) * step / warmup_iters + wf)
        return lr0 * (0.1 ** (step / (decay * 1000)))

    for step in (0, 700, wi - 1, wi, wi + 1, 123456):           # warm-up steps, the boundary, decay steps
        assert f(lr0, step, decay, wi, wf) == expected(step, wi), step
        assert f(lr0, step, decay) == expected(step, -1), step  # no warm-up (the default)
    assert f(lr0, 0, decay, wi, wf) == lr0 * wf and f(lr0, 250000, decay) == pytest.approx(lr0 * 0.1, rel=1e-15)
    assert f(lr0, wi - 1, decay, wi, wf) < lr0 and f(lr0, wi, decay, wi, wf) == lr0 * 0.1 ** (wi / 250000)
