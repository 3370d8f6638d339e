"""The float64 restatement of the PDRF level of any shape (tests/voxel_generic_ref.py) against golden G41: the reference's own
VoxelNeRFBase layers in float64 (tools/gen_golden_voxel_generic.py), eight runs over six level shapes.  Both sides are float64, so the
bound is 1e-12 on raw and the geo rows and 1e-9 of each gradient's norm.  Also the two input conditions the GPU tests rely on, asserted
on the reference alone: the sign balance of sigma and the cap on the tie samples."""
import numpy as np
import pytest

import voxel_generic_ref as G
from conftest import load_golden
from torch_restatement import grad_summary


@pytest.fixture(scope="module")
def g41():
    return load_golden("G41_voxel_generic")


@pytest.mark.parametrize("name", list(G.CASES))
def test_restatement_matches_the_reference_golden(g41, name):
    e = G.evaluate(name, grads=True, zero_ties=False)
    si = g41[f"{name}.sample_idx"]             # raw at 256 seeded samples, whole geo rows at every 16th of them
    assert len(si) == min(256, e["raw"].shape[0])
    assert np.abs(e["raw"].numpy()[si] - g41[f"{name}.raw"]).max() < 1e-12
    assert e["geo"].shape[1] == G.CASES[name][1] == g41[f"{name}.geo"].shape[1]
    assert np.abs(e["geo"].numpy()[si[::16]] - g41[f"{name}.geo"]).max() < 1e-12
    keys = G.net_keys(name)
    assert list(g41[f"{name}.names"]) == keys == list(e["grads"])          # the reference's named_parameters(), in its order
    ci = list(G.CASES).index(name)
    for i, key in enumerate(keys):
        g = e["grads"][key].numpy()
        sm, _ = grad_summary(g, 7000 + 100 * ci + i)
        ref = g41[f"{name}.{key}.summary"]
        assert max(abs(sm[0] - ref[0]), abs(sm[1] - ref[1])) < 1e-9 * ref[0], (key, sm, ref)
        assert np.abs(g.reshape(-1)[g41[f"{name}.{key}.elem_idx"]] - g41[f"{name}.{key}.elem_val"]).max() < 1e-9 * ref[0], key


@pytest.mark.parametrize("name", list(G.CASES))
def test_input_conditions_hold_on_the_reference(name):
    e = G.evaluate(name)
    tie = float(e["tie"].double().mean())
    print(f"case {name}: sigma > 0 on {100 * e['share']:.1f} % of the samples, {100 * tie:.2f} % within {G.TAU:g} of a ReLU tie, A = {e['A']:.3f}")
    assert 0.25 <= e["share"] <= 0.75
    assert tie <= G.TIE_CAP
