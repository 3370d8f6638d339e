"""The two feature outputs of the float64 restatement tests/nerf_generic_ref.py GenericNerf (out["feature1"] = the feature_linear output,
extract_feature="after_linear"; out["feature2"] = the ReLU output of the last pts_linears layer, "before_linear") against golden G45's
`feat.*` arrays: the reference's own NeRF.eval in float64 with either setting (tools/gen_golden_nerf_awp.py), case `a`.  Both sides are
float64: 1e-12.  The restatement is the reference of tests/test_gpu_nerf_feature_train.py."""
import numpy as np
import torch

import nerf_generic_ref as G
from conftest import load_golden


def test_feature_outputs_match_the_reference_golden():
    g = load_golden("G45_nerf_awp_train")
    rb, z, _ = G.case_inputs("a")
    net = G.case_net("a")
    out = {}
    with torch.no_grad():
        raw = net(*G.positions(rb, z), out=out)
    assert g["feat.after_linear"].dtype == np.float64 and g["feat.after_linear"].shape == (z.size, G.CASES["a"][1])
    assert np.abs(raw.numpy() - g["feat.raw"]).max() < 1e-12
    e1 = np.abs(out["feature1"].numpy() - g["feat.after_linear"]).max()
    e2 = np.abs(out["feature2"].numpy() - g["feat.before_linear"]).max()
    print(f"feature1 vs the reference's after_linear feature: {e1:.1e}; feature2 vs before_linear: {e2:.1e}")
    assert e1 < 1e-12 and e2 < 1e-12
    assert np.abs(g["feat.after_linear"] - g["feat.before_linear"]).max() > 1e-2            # two different tensors
    assert (g["feat.before_linear"] >= 0).all() and (g["feat.after_linear"] < 0).any()      # one is a ReLU output, the other is not


def test_training_call_golden_shape():
    """what tests/test_gpu_nerf_awp_train_call.py relies on: 8 pixels x 5 sub-exposures, 32 merged samples, every NeRF tensor's gradient"""
    g = load_golden("G45_nerf_awp_train")
    R, P = g["weight"].shape
    assert (R, P) == (8, 5) and g["new_rays"].shape == (R, P, 3, 2) and g["awp_in_z_vals"].shape == (R * P, 32)
    keys = [k[2:-8] for k in g if k.startswith("g.mlp_") and k.endswith(".summary")]
    assert len(keys) == 2 * (2 * 4 + 8) and all(float(g[f"g.{k}.summary"][0]) > 0 for k in keys)
    assert g["g.awp.sample_feature_embed_layer.0.weight"].shape == (64, 64)
