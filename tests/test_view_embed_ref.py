"""CPU-only: the float64 restatement tests/view_embed_ref.py of ViewEmbeddingMLP (networks/embedding.py:35-62) reproduces what the
reference's real module, run in float64 on the CPU, left in golden G40: the table and every parameter gradient to 1e-12 of the norm."""
import numpy as np
import pytest

from conftest import load_golden
import view_embed_ref as VR


@pytest.mark.parametrize("tag", VR.G40_CASES)
def test_restatement_reproduces_the_float64_reference(tag):
    c = VR.g40_case(load_golden("G40_view_embed_mlp"), tag)
    ref = VR.run(c["params"], c["skips"], c["ids"], c["proj"])
    a = c["alone"]
    assert set(ref["grads"]) == set(a["g64"]) == set(VR.param_keys(c["D"]))
    errs = {"table": VR.rel_l2(ref["table"], a["out64"]["table"])}
    errs.update({k: VR.rel_l2(ref["grads"][k], a["g64"][k]) for k in a["g64"]})
    print(tag, {k: f"{v:.1e}" for k, v in errs.items()})
    assert a["out64"]["table"].dtype == np.float64 and ref["table"].shape == (c["n_img"], c["W"])
    assert max(errs.values()) <= 1e-12, errs
    if c["absent"] is not None:
        assert c["absent"] not in c["ids"] and not ref["grads"]["img_embed"][c["absent"]].any() and not a["g64"]["img_embed"][c["absent"]].any()


@pytest.mark.parametrize("tag", VR.G40_CASES)
def test_no_relu_sits_on_the_fence(tag):
    """the generator's condition, recomputed: a float32 evaluation of the case cannot decide a unit differently from float64"""
    g = load_golden("G40_view_embed_mlp")
    c = VR.g40_case(g, tag)
    margin, thr = VR.fence_margin(c["params"], c["skips"])
    assert margin >= thr and np.allclose([margin, thr], g[tag + ".fence"], rtol=1e-9)


def test_the_skip_concatenation_puts_the_embedding_first():
    """embedding.py:59-60: with layer 1 = identity on the embedding columns (and zero on the hidden ones) the output is relu(embedding)"""
    rs = np.random.RandomState(0)
    E, W = 3, 3
    p = {"img_embed": rs.standard_normal((4, E)), "view_embed_linears.0.weight": rs.standard_normal((W, E)), "view_embed_linears.0.bias": np.zeros(W),
         "view_embed_linears.1.weight": np.concatenate([np.eye(E), np.zeros((W, W))], 1), "view_embed_linears.1.bias": np.zeros(W)}
    assert np.array_equal(VR.forward(p, [0]), np.maximum(p["img_embed"], 0.0))
