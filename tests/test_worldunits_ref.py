"""CPU: what m2s_records_to_world_units is for, shown with the oracle and the committed restatements (tests/worldunits_ref.py, merge_ref.py,
lod_ref.py).  The oracle's unit quad at R = 64 is 4096 records of stored edge 1.0 — R times the h = 1/64 the viewer draws.  Read as
stored, a parent's edges hardly grow and no camera gets a mixed cut (Limits); divided by R first, the chain is the quadtree
the merge pass was built for and the cuts are mixed."""
import numpy as np
import pytest

import lod_ref as lr
import merge_ref as mr
import worldunits_ref as wr
from mesh2splat_amd import _lib, synth

F = np.float32
R = 64
CHAIN = (4, 5, 6, 7, 8, 9, 10)
CAMERAS = ((0.0, 0.0, 0.3), (0.5, 0.5, 2.0), (0.5, 0.5, 8.0), (-1.0, 0.5, 0.3))
TAUS = (1.0, 2.0, 4.0)
FOCAL = 154.51


def chain(rec, levels=CHAIN, max_group=4, dot=0.5):
    """the merges one after the other, as m2s_lod_build runs them (a step that merges nothing adds no level)
    -> (the levels' records, parent, first)"""
    out, maps, pending = [rec], [], None
    for lv in levels:
        nxt, m, counts, _ = mr.merge(out[-1] if pending is None else pending[0], lv, max_group, dot)
        m = m if pending is None else m[pending[1]]
        if counts["after"] == len(out[-1]):
            pending = (nxt, m)
            continue
        pending = None
        out.append(nxt)
        maps.append(m)
    parent, first = lr.link(maps, [len(v) for v in out])
    return out, parent, first


@pytest.fixture(scope="module")
def quad(oracle):
    total, rec, _ = oracle.convert(synth.unit_quad(), R)
    assert total == len(rec) == R * R and (rec[:, 8:10] == F(1)).all()
    return np.ascontiguousarray(rec, F)


@pytest.fixture(scope="module")
def stored(quad):
    return chain(quad)


@pytest.fixture(scope="module")
def world(quad):
    return chain(wr.to_world_units(quad, R))


def longest(level):
    return lr.bounds(level)[:, 3]


def test_restatement_divides_the_scales_and_nothing_else(quad):
    got = wr.to_world_units(quad, R)
    assert got.dtype == F and (got[:, 8:10] == F(1 / 64)).all() and (got[:, 10] == quad[:, 10] / F(64)).all()
    keep = [k for k in range(24) if k not in (8, 9, 10)]
    assert np.array_equal(got[:, keep].view(np.uint32), quad[:, keep].view(np.uint32))
    for noop in (0, 1):
        assert np.array_equal(wr.to_world_units(quad, noop).view(np.uint32), quad.view(np.uint32))
    odd = wr.to_world_units(quad, 48)
    assert (odd[:, 8] == F(1) / F(48)).all()


def test_world_units_make_the_chain_a_quadtree(world):
    levels, parent, first = world
    h = F(1) / F(R)
    print("world units, nodes per level:", [len(v) for v in levels])
    assert len(levels) >= 3 and len(levels[0]) == R * R
    # The first two levels of the chain have a longest edge of exactly 2h and 4h (dyadic operands: fp32 equality).  They come from the
    # steps at merge levels 5 and 6: the cells of level 4, 64 per axis, hold one record each here, and that step adds no level.
    assert mr.merge(levels[0], 4, 4, 0.5)[2]["after"] == R * R and mr.merge(levels[0], 5, 4, 0.5)[2]["after"] == len(levels[1]) == 1088
    assert longest(levels[1]).max() == F(2) * h == F(0.03125)
    assert longest(levels[2]).max() == F(4) * h == F(0.0625)
    assert all(len(a) > len(b) for a, b in zip(levels, levels[1:]))


def test_stored_units_hardly_grow(stored):
    """DESIGN 5.19's figure is the level's MEDIAN longest edge (1.0, 1.00037, 1.0018, ...: "1.0004 against the 2 that a 2 x 2 block
    needs"); the largest edge of a level, printed beside it, reaches 1.23 on the last level, where a segment straddles a cell border."""
    levels, parent, first = stored
    print("stored units, median longest edge per level:", [float(np.median(longest(v))) for v in levels])
    print("stored units, largest edge per level:", [float(longest(v).max()) for v in levels])
    assert (longest(levels[0]) == F(1)).all() and len(levels) >= 3
    for lv in levels[1:]:
        assert 1.0 <= float(np.median(longest(lv))) <= 1.01
        assert float(longest(lv).max()) < 2.0                                       # no node reaches even the first quadtree level's edge


def test_cuts_are_mixed_in_world_units_and_all_leaves_in_stored_units(stored, world):
    for name, (levels, parent, first) in (("stored", stored), ("world", world)):
        b = lr.bounds(np.concatenate(levels))
        for cam in CAMERAS:
            mixed = 0
            for tau in TAUS:
                sel = lr.select(b, parent, first, cam, FOCAL, tau)
                print(f"{name} cam={cam} tau={tau}: per level {sel['per_level']}")
                assert lr.cut_ok(parent, first, sel["flags"])
                if name == "stored":
                    assert sel["per_level"][0] == sel["counts"]["selected"] == R * R
                mixed += sum(1 for v in sel["per_level"] if v) >= 2
            assert name == "stored" or mixed >= 1, cam


def test_symbol_list_has_the_new_names():
    assert "m2s_records_to_world_units" in _lib.EXPORTS and "m2s_last_world_units_ms" in _lib.EXPORTS
