"""CPU-only: the float64 restatement tests/sparse_blur_ref.py against the reference's recorded float32 results (golden G39: BlurModel with
ViewEmbedding 'param', kernel_type DSK and PBE), within the reference's own float32 error (ref_f32_err: float32 against the same module in
float64) times 4."""
import numpy as np
import pytest

from conftest import load_golden
import sparse_blur_ref as SR

FACTOR = 4.0


@pytest.mark.parametrize("tag", SR.G39_CASES)
def test_restatement_matches_the_recorded_reference(tag):
    g = load_golden("G39_sparse_blur")
    c = SR.g39_case(g, tag)
    ref = SR.g39_reference(g, tag)
    assert set(ref["grads"]) == set(SR.param_keys(c["cfg"])) == set(c["params"]) - {"poses"}
    for k in ("new_rays", "weight") + (("align",) if c["cfg"]["kernel_type"] == "DSK" else ()):
        e = float(np.abs(ref[k] - c["out"][k].reshape(ref[k].shape)).max())
        print(f"G39 {tag} {k}: {e:.2e} (bound {FACTOR:.0f} x {c['err_out'][k]:.2e})")
        assert e <= FACTOR * c["err_out"][k], (k, e)
    assert (ref["align"] is None) == (c["cfg"]["kernel_type"] == "PBE") == ("align" not in c["out"])
    assert np.array_equal(ref["img_embed"].astype(np.float32), c["out"]["img_embed"])
    grads = dict(ref["grads"], **({"feats": ref["d_feats"]} if c["feats"] is not None else {}))
    assert set(grads) == set(c["grads"])
    for k, v in grads.items():
        e = SR.rel_l2(c["grads"][k], v)
        print(f"G39 {tag} d {k}: {e:.2e} of the norm (bound {FACTOR:.0f} x {c['err_g'][k]:.2e})")
        assert e <= FACTOR * c["err_g"][k], (k, e)
    for k in ("pattern_pos", "pattern_trans", "img_embed.img_embed"):
        if k in grads and not c["cfg"]["isglobal"] or k == "img_embed.img_embed":
            assert not grads[k][SR.ABSENT_IMAGE].any(), k


def test_pbe_without_feats():
    g = load_golden("G39_sparse_blur")
    c = SR.g39_case(g, "pbe")
    ref = SR.run(c["params"], c["cfg"], c["H"], c["W"], c["K4"], c["ids"], c["rays_x"], c["rays_y"], c["poses"], c["noise"], c["proj"])
    for k in ("new_rays", "weight"):
        e = float(np.abs(ref[k] - g["pbe.out_nofeats." + k]).max())
        bound = FACTOR * float(g["pbe.ref_f32_err.out_nofeats." + k])
        print(f"G39 pbe feats=None {k}: {e:.2e} (bound {bound:.2e})")
        assert e <= bound
    fx, fy, cx, cy = c["K4"]                                         # point 0 of PBE carries no offset: the pixel's own ray
    d0 = np.stack([(c["rays_x"][:, 0] - cx) / fx, -(c["rays_y"][:, 0] - cy) / fy, -np.ones(len(c["ids"]))], -1)
    assert np.allclose(ref["new_rays"][:, 0, :, 1], np.einsum("rjk,rk->rj", c["poses"][:, :, :3].astype(np.float64), d0), atol=1e-12)
    assert np.array_equal(ref["new_rays"][:, 0, :, 0], c["poses"][:, :, 3].astype(np.float64))
