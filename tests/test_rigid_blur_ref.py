"""CPU-only: the float64 restatement of the rigid blur kernel network (tests/rigid_blur_ref.py: all motions at once, closed-form
Rodrigues with series coefficients at small angles) against golden G37 = the reference's real RigidBlurringModel + ViewEmbedding in
float32.  The bound is the fixture's own record of how far the reference's float32 results are from the reference run in float64
(ref_f32_err): a restatement that is the same function lands within it; one with a wrong motion layout, sign or coefficient misses it by
orders of magnitude (the last test).

The recorded number is |float32 - reference in float64|; the test measures |float32 - restatement in float64|.  The two float64
evaluations run the same function in a different operation order and differ by float64 rounding (measured: 2e-16 absolute on the outputs,
1e-10 of a recorded error), so the comparison carries F64_SLACK = one part in a million of the recorded error and nothing else."""
import numpy as np
import pytest

from conftest import load_golden
import rigid_blur_ref as RR

F64_SLACK = 1.0 + 1e-6


@pytest.mark.parametrize("tag", RR.G37_CASES)
def test_restatement_matches_the_reference_G37(tag):
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, tag)
    r = RR.g37_reference(g, tag)
    assert np.array_equal(r["img_embed"].astype(np.float32), c["out"]["img_embed"])
    for k in ("new_rays", "weight"):
        assert c["out"][k].dtype == np.float32 and c["out"][k].shape == r[k].shape
        e = float(np.abs(c["out"][k].astype(np.float64) - r[k]).max())
        print(f"G37 {tag} {k}: reference float32 vs restatement {e:.2e} (recorded float32 error {c['err_out'][k]:.2e})")
        assert e <= c["err_out"][k] * F64_SLACK, (k, e, c["err_out"][k])
    got = dict(r["grads"], rays=r["d_rays"])
    assert set(got) == set(c["grads"]) == set(c["err_g"])
    for k, ref in c["grads"].items():
        e = RR.rel_l2(ref, got[k])
        print(f"G37 {tag} d {k}: reference float32 vs restatement {e:.2e} of the norm (recorded {c['err_g'][k]:.2e})")
        assert e <= c["err_g"][k] * F64_SLACK, (k, e, c["err_g"][k])
    assert not got["view_embed_module.img_embed"][RR.ABSENT_IMAGE].any() and RR.ABSENT_IMAGE not in c["ids"]


def test_fixture_is_what_the_issue_describes():
    g = load_golden("G37_rigid_blur")
    lo, hi = g["regular.theta_range"]
    assert 5e-3 < lo and hi < 5e-2
    lo, hi = g["small.theta_range"]
    assert 1e-5 < lo and hi < 1e-3                                    # float32 1 - cos(theta) is 0 or 1 ulp here
    c = RR.g37_case(g, "odd")
    assert not c["use_origin"] and c["M"] == 4 and c["rays"].shape[0] == 67 and (c["ids"] == 5).sum() * 2 > 67
    assert {k[len("train_call.sd."):] for k in g if k.startswith("train_call.sd.")} == set(RR.PARAM_KEYS)


def test_the_bound_tells_a_wrong_restatement_apart():
    """motion-major instead of component-major r / v columns (blurmodel.py:52-53 reshapes [R, 3 M] to [R, 3, M]): far outside the bound"""
    g = load_golden("G37_rigid_blur")
    c = RR.g37_case(g, "regular")
    T = lambda a: __import__("torch").tensor(a, dtype=__import__("torch").float64)
    p = {k: T(v) for k, v in c["params"].items()}
    perm = np.arange(3 * c["M"]).reshape(c["M"], 3).T.reshape(-1)
    for k in ("r_linear.weight", "r_linear.bias", "v_linear.weight", "v_linear.bias"):
        p[k] = p[k][perm]
    x = p["view_embed_module.img_embed"][c["ids"]]
    new_rays, _ = RR.forward(p, T(c["rays"]), x, c["M"], c["use_origin"], c["rv_window"])
    assert np.abs(new_rays.numpy() - c["out"]["new_rays"]).max() > 1e3 * c["err_out"]["new_rays"]
