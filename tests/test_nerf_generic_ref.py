"""The float64 restatement of the generic NeRF network (tests/nerf_generic_ref.py) against golden G40: the reference's own NeRF class in
float64 (tools/gen_golden_nerf_generic.py), six networks of different depth, width, skip and frequency counts.  Both sides are float64,
so the bound is 1e-9 of each gradient's norm.  Also the cap on the samples whose d raw the GPU tests zero (ReLU ties)."""
import numpy as np
import pytest
import torch

import nerf_generic_ref as G
from conftest import load_golden
from torch_restatement import check_grad_elements, grad_summary


@pytest.fixture(scope="module")
def g40():
    return load_golden("G40_nerf_generic_grads")


@pytest.mark.parametrize("name", list(G.CASES))
def test_restatement_matches_the_reference_golden(g40, name):
    rb, z, d_raw = G.case_inputs(name)
    net = G.case_net(name)
    pts, dirs = G.positions(rb, z)
    pre = {}
    raw = net(pts, dirs, pre)
    D = G.CASES[name][0]
    assert set(pre) == {f"h{l}" for l in range(D)} | {"hv"}
    assert np.abs(raw.detach().numpy() - g40[f"{name}.raw"]).max() < 1e-12
    (raw * torch.tensor(d_raw, dtype=torch.float64).reshape(-1, 4)).sum().backward()
    ci = list(G.CASES).index(name)
    keys = list(G.case_state_dict(name))
    assert {k for k in g40 if k.startswith(name + ".") and k.endswith(".summary")} == {f"{name}.{k}.summary" for k in keys}
    for i, key in enumerate(keys):
        g = net.p[key.replace(".", "_")].grad.numpy()
        sm, _ = grad_summary(g, 7000 + 100 * ci + i)
        ref = g40[f"{name}.{key}.summary"]
        assert max(abs(sm[0] - ref[0]), abs(sm[1] - ref[1])) < 1e-9 * ref[0], (key, sm, ref)
        val = g40[f"{name}.{key}.elem_val"]
        assert np.abs(g.reshape(-1)[g40[f"{name}.{key}.elem_idx"]] - val).max() < 1e-9 * ref[0], key


@pytest.mark.parametrize("name", list(G.CASES))
def test_tie_samples_stay_under_the_cap(name):
    raw, grads, d_raw, frac = G.case_reference(name)
    print(f"case {name}: {100 * frac:.2f} % of the samples have a float64 pre-activation within {G.TAU:g} of zero")
    assert frac <= G.TIE_CAP
    assert (np.abs(d_raw).reshape(-1, 4).max(-1) == 0).mean() == pytest.approx(frac, abs=1e-12)
