"""CPU-only: the numpy restatement of the event tables (tests/event_tables_ref.py) against the C oracle (oracle.event_tables /
oracle.compute_successor) on every edge case tests/test_gpu_event_tables_edges.py feeds the kernels, and against golden G34 = the reference's
own load_event_data.  Two references written independently that agree bit for bit, sign bits of id_to_coords included, are what the GPU
tests then hold the kernels to."""
import numpy as np
import pytest

from conftest import load_golden
import event_tables_ref as R
from oracle import oracle as O

TMIN, TMAX = float(R.KEY_T.min()), float(R.KEY_T.max())
COORD, RANGE, POL, SUCC = R.coord_cases(), R.range_cases(), R.polarity_cases(), R.successor_cases()


def oracle_tables(c, check=None):
    return O.event_tables(c["x"], c["y"], c["t"], c["p"], c["h"], c["w"], TMIN, TMAX, ev_map=c["ev_map"], color_events=True,
                          check=c["check"] if check is None else check)


def both(c, check=None):
    ref, orc = R.run(c, check=check), oracle_tables(c, check=check)
    assert R.mismatches(orc, ref) == []
    return ref


def color_of(tb, x, y):
    """the colour row of the coordinate equal (by value) to (x, y)"""
    hit = np.flatnonzero((tb["id_to_coords"][:, 0] == x) & (tb["id_to_coords"][:, 1] == y))
    assert hit.shape[0] == 1
    return tb["id_to_color_map"][hit[0]].astype(np.uint8).tolist()


@pytest.mark.parametrize("name", sorted(COORD))
def test_coordinate_cases_equal_the_oracle(name):
    c = COORD[name]
    tb = both(c)
    n, hw = c["x"].shape[0], c["h"] * c["w"]
    assert tb["id_to_coords"].shape[0] <= n + hw and tb["noev_coord_ids"].shape[0] <= hw
    if name == "n0":                                          # every pixel silent: the ids are the pixels in byte order, no event row
        i2c = tb["id_to_coords"]
        assert i2c.shape == (hw, 2) and tb["events"].shape == (0, 4) and tb["noev_coord_ids"].shape == (hw,)
        be = np.ascontiguousarray(i2c).view(np.uint8).reshape(hw, 16)
        assert all(bytes(be[k]) < bytes(be[k + 1]) for k in range(hw - 1))
        assert np.array_equal(i2c[tb["noev_coord_ids"]], np.stack([np.arange(hw) % c["w"], np.arange(hw) // c["w"]], -1))
    if name == "n1":
        assert tb["events"].shape == (1, 4) and tb["noev_coord_ids"].shape == (hw - 1,) and tb["events_with_successor_idx"].shape == (0,)
    if name == "every_pixel":
        assert tb["noev_coord_ids"].shape == (0,) and tb["id_to_coords"].shape == (hw, 2)
    if name.startswith("one_pixel"):
        assert tb["id_to_coords"].shape == (hw, 2) and np.all(tb["events"][:, 0] == tb["events"][0, 0])
        assert np.array_equal(tb["events_num_successors"], np.arange(299, -1, -1))
    if name.startswith("m"):
        assert n + hw == int(name[1:4])
    if name == "rounding":                                     # half to even and the clip: these pixels carry an event, the rest is silent
        struck = {(0, 0), (2, 2), (0, 4), (2, 4), (3, 5), (1, 2), (2, 0), (0, 2), (2, 3)}       # (row, column)
        silent = {(int(y), int(x)) for x, y in tb["id_to_coords"][tb["noev_coord_ids"]]}
        assert silent == {(j, i) for j in range(c["h"]) for i in range(c["w"])} - struck
        assert not tb["intcoords"]


@pytest.mark.parametrize("name", ["signed_zero_map_neg", "signed_zero_map_pos"])
def test_signed_zero_matches_by_value(name):
    """loader_events.py:229-232: the dict finds 0.0 under -0.0 and the other way round, and the last pixel in raster order wins"""
    c = COORD[name]
    for tb in (R.run(c), oracle_tables(c)):
        assert color_of(tb, 0.0, 0.0) == [1, 0, 0]                              # pixel (0, 0): red
        assert color_of(tb, 1.25, 1.125) == [1, 0, 0]                           # pixel (2, 4)'s red, not pixel (1, 1)'s blue
        zero = tb["id_to_coords"][(tb["id_to_coords"][:, 0] == 0) & (tb["id_to_coords"][:, 1] == 0)]
        assert bool(np.signbit(zero[0, 0])) == (name == "signed_zero_map_pos")  # the sign of the EVENT's zero is kept


@pytest.mark.parametrize("name", sorted(RANGE))
def test_range_cases_equal_the_oracle(name):
    c = RANGE[name]
    tb = both(c)
    inside = (c["t"] >= TMIN) & (c["t"] <= TMAX)
    assert tb["events"].shape == (int(inside.sum()), 4) and np.array_equal(tb["events"][:, 1], c["t"][inside])
    if name == "ends":
        assert tb["events"].shape[0] == 5 and (tb["events"][:, 1] == TMIN).sum() == 2 and (tb["events"][:, 1] == TMAX).sum() == 2
    if name == "all_outside":
        assert tb["events"].shape == (0, 4)


@pytest.mark.parametrize("name", sorted(POL))
def test_polarity_cases_equal_the_oracle(name):
    c, raises = POL[name]
    if raises:
        with pytest.raises(ValueError, match="206"):
            R.run(c)
        with pytest.raises(ValueError, match="206"):
            oracle_tables(c)
    tb = both(c, check=False)
    got = sorted(set(tb["events"][:, 2].tolist()))
    want = {"01": [-1, 1], "m11": [-1, 1], "m101": [-1, 0, 1], "1": [1], "0": [-1], "m1": [-1], "012": [-1, 1, 2], "outside3": [-1, 1]}[name]
    assert got == want


def test_error_cases_raise_in_both():
    c = R.unmapped_case()
    for f in (R.run, oracle_tables):
        with pytest.raises(ValueError, match="colour"):
            f(c)
    tb = both(c, check=False)
    assert color_of(tb, 2.0, 0.25) == [0, 0, 0]                       # the event on pixel (0, 2): no map entry, no colour
    with_map = dict(COORD["m255_int"], ev_map=R.identity_map(3, 5))           # integer coordinates, and an ev_map given (:216-217)
    without = dict(COORD["m255_flt"], ev_map=None)                            # float coordinates without one (:221-222)
    past = dict(COORD["m255_int"])                                            # an integer coordinate at x = w (:199)
    past["x"] = past["x"].copy()
    past["x"][17] = past["w"]
    for f in (R.run, oracle_tables):
        with pytest.raises(ValueError, match="216"):
            f(with_map)
        with pytest.raises(ValueError, match="221"):
            f(without)
        with pytest.raises(IndexError):
            f(past)


@pytest.mark.parametrize("name", sorted(SUCC))
def test_successor_cases_equal_the_oracle(name):
    ids, hw = SUCC[name]
    ref, orc = R.successor(ids, hw), O.compute_successor(ids, hw)
    for a, b in zip(ref, orc):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    succ, nsucc, latest, first = ref
    seen = 0
    for p in range(hw):                                        # the chain from latest[p] visits exactly p's events, in stream order
        chain = R.chain_of(p, succ, nsucc, latest)
        assert chain == np.flatnonzero(ids == p).tolist()
        assert (first[p] == chain[-1]) if chain else (latest[p] == -1 and first[p] == -1)
        seen += len(chain)
    assert seen == ids.shape[0]
    for bad in ([-1], [hw]):
        with pytest.raises(IndexError):
            R.successor(np.array(bad, np.int32), hw)
        with pytest.raises(IndexError):
            O.compute_successor(np.array(bad, np.int32), hw)


@pytest.mark.parametrize("tag", ["int", "flt"])
def test_restatement_matches_golden_G34(tag):
    """the reference's own load_event_data on the generator's arrays (data/loader_events.py:150-257)"""
    from test_oracle_golden import check_event_tables
    g = load_golden("G34_event_tables")
    h, w = (int(v) for v in g[f"{tag}_hw"])
    acc = [int(v) for v in g[f"{tag}_acc"]]
    min_step = max(acc[0], acc[2]) if tuple(acc[:2]) != (0, 0) else 0
    ev_map = (g["flt_inv_mapx"], g["flt_inv_mapy"]) if tag == "flt" else None
    got = R.tables(g[f"{tag}_x"], g[f"{tag}_y"], g[f"{tag}_t"], g[f"{tag}_p"], h, w, float(g[f"{tag}_key_t"].min()), float(g[f"{tag}_key_t"].max()),
                   ev_map=ev_map, color_events=True, min_step=min_step)
    check_event_tables(got, g, tag)
    if tag == "int":
        assert np.array_equal(got["coords_to_id"], g["int_coords_to_id"])
