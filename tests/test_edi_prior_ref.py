"""CPU-only: the float64 restatement of the EDI prior table (tests/edi_prior_ref.py) against golden G36 = the reference's own
LLFFEventsDataset.compute_edi_prior (data/loader_events.py:99-131) on two inputs, and what the fixture is worth: it holds events exactly on
the start, interior and end boundaries, and a restatement with either edge of the window made exclusive misses it by far."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
import edi_prior_ref as R

LARGEST_FIXTURE = 861_461          # G33_train_trajectory.npz: no fixture is larger


def g36_case(tag):
    """-> (inputs of the case, {name: (stored reference result, index into the [n, H, W, 3] result)})"""
    g = load_golden("G36_edi_prior")
    if tag == "int":
        ev = np.concatenate([g["int_events"], np.zeros((g["int_events"].shape[0], 1))], -1)
        h, w = g["int_images"].shape[1:3]
        gx, gy = np.meshgrid(np.arange(w), np.arange(h))
        d = {"events": ev, "id_to_coords": np.stack([gx.reshape(-1), gy.reshape(-1)], -1).astype(np.float64), "tms_start": g["int_tms_start"],
             "tms_end": g["int_tms_end"], "images": g["int_images"], "steps": int(g["int_args"][0]), "cpos": float(g["int_args"][1]),
             "cneg": float(g["int_args"][2])}
        return d, {"prior": (g["int_prior"], np.s_[:])}
    d = R.g36_flt_inputs()
    return d, {"c0": (g["flt_prior_c0"], np.s_[..., 0]), "c12_rows": (g["flt_prior_c12_rows"], np.s_[:, ::R.G36_FLT_ROWS, :, 1:])}


def ref_of(d, rule="closed"):
    return R.edi_prior_ref(d["events"], d["id_to_coords"], d["tms_start"], d["tms_end"], d["images"], d["steps"], d["cpos"], d["cneg"], rule=rule)


@pytest.mark.parametrize("tag", ["int", "flt"])
def test_restatement_matches_the_reference_G36(tag):
    """every stored element of the reference's float32 result within 2 u E of the float64 restatement"""
    d, stored = g36_case(tag)
    r = ref_of(d)
    for name, (gold, sel) in stored.items():
        assert gold.dtype == np.float32 and gold.shape == r["prior"][sel].shape
        worst = R.worst_ratio(gold, r["prior"][sel], r["E"][sel])
        print(f"G36 {tag} {name}: the reference's worst err / (u E) = {worst:.3f} over {gold.size} elements")
        assert np.isfinite(gold).all() and worst <= R.K


def boundary_events(d):
    """indices of the events exactly on a start / interior / end boundary of an exposure, and 1 microsecond outside start / end"""
    t = d["events"][:, 1]
    kinds = {k: [] for k in ("start", "interior", "end", "before", "after")}
    for a, b in zip(d["tms_start"], d["tms_end"]):
        bd = np.linspace(a, b, d["steps"])
        kinds["start"].append(np.nonzero(t == bd[0])[0])
        kinds["interior"].append(np.nonzero(np.isin(t, bd[1:-1]))[0])
        kinds["end"].append(np.nonzero(t == bd[-1])[0])
        kinds["before"].append(np.nonzero(t == a - 1)[0])
        kinds["after"].append(np.nonzero(t == b + 1)[0])
    return {k: np.concatenate(v) for k, v in kinds.items()}


def test_fixture_holds_boundary_events_of_every_kind():
    d, _ = g36_case("int")
    kinds = boundary_events(d)
    print("G36 int: events", {k: len(v) for k, v in kinds.items()})
    for k, v in kinds.items():
        assert len(v) >= 3 * 4, k                                   # several per exposure
    assert np.all(d["events"][:, 1] == np.round(d["events"][:, 1])) and np.all((d["tms_end"] - d["tms_start"]) % 8 == 0)
    # the 'flt' case: taps off the right and the bottom edge, no negative coordinate, dozens of taps on one pixel in one window
    f, _ = g36_case("flt")
    xy = f["id_to_coords"][f["events"][:, 0].astype(np.int64)]
    h, w = f["images"].shape[1:3]
    assert (xy[:, 0] > w - 1).sum() > 100 and (xy[:, 1] > h - 1).sum() > 100 and xy.min() >= 0
    left, right = R.windows(f["events"][:, 1], np.linspace(f["tms_start"][0], f["tms_end"][0], f["steps"]))
    assert (right[1:] - left[:-1]).min() > 2000
    e = xy[left[0]:right[1]]
    assert R.splat(e[:, 0], e[:, 1], h, w)[1].max() >= 24


@pytest.mark.parametrize("rule,dropped", [("open_right", ("interior", "end")), ("open_left", ("start", "interior"))])
def test_fixture_tells_the_window_rule(rule, dropped):
    """with an exclusive right (left) edge the events on an interior or the end (start) boundary leave a window: at their pixels the
    result is more than 100 bounds away from the reference's"""
    d, stored = g36_case("int")
    gold = stored["prior"][0]
    wrong = ref_of(d, rule)
    kinds = boundary_events(d)
    h, w = gold.shape[1:3]
    n_checked = 0
    for i, (a, b) in enumerate(zip(d["tms_start"], d["tms_end"])):
        t = d["events"][:, 1]
        idx = np.concatenate([kinds[k] for k in dropped])
        idx = idx[(t[idx] >= a) & (t[idx] <= b)]
        pix = np.unique(d["events"][idx, 0].astype(np.int64))
        ratio = np.abs(gold[i].reshape(h * w, 3)[pix] - wrong["prior"][i].reshape(h * w, 3)[pix]) / (R.K * R.U * wrong["E"][i].reshape(h * w, 3)[pix])
        print(f"G36 int, rule {rule}, exposure {i}: {len(pix)} pixels of boundary events, |wrong - G36| / (2 u E) from {ratio.min():.3g} to {ratio.max():.3g}")
        assert ratio.min() > 100
        n_checked += len(pix)
    assert n_checked >= 30
    # and away from those pixels the two rules agree: the difference IS the boundary events
    assert R.worst_ratio(gold, wrong["prior"], wrong["E"]) > 100 * R.K


def test_fixture_size():
    size = os.path.getsize(os.path.join(GOLDEN, "G36_edi_prior.npz"))
    assert size <= LARGEST_FIXTURE, size
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) <= LARGEST_FIXTURE for f in os.listdir(GOLDEN))
    g = load_golden("G36_edi_prior")
    assert all(v.dtype.kind in "fiu" for v in g.values())          # numeric arrays only
