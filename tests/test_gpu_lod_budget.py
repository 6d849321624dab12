"""-m gpu: m2s_lod_select_budget (Converter.lod_select_budget) against its numpy restatement (tests/lod_budget_ref.py, held to the cut's
own restatement by tests/test_lod_budget_ref.py) and against Converter.lod_select at the returned tau_px on a second context.  Everything
is compared for equality: the bits of tau_px, met, selected_finer, counts, per-level counts, node indices, record bytes."""
import ctypes as C

import numpy as np
import pytest

import lod_budget_ref as br
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod, synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams

pytestmark = pytest.mark.gpu
F = np.float32
CHAINS = ((0,), (3, 10), tuple(range(1, 11)))
FOCAL, NEAR = 600.0, 0.05
SEEN = {"cuts": 0, "mixed": 0, "unmet": 0, "floor": 0, "jump": 0, "special_inner": 0}   # over the module: asserted by the last test


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(hiplib):
    c = Converter(0)
    yield c
    c.close()


def special_records(n, seed):
    """the crafted records of the level-of-detail tests (shared positions, zero scales, three invalid records); from 65 records on also
    four records on their own far from the others whose longer edge is 0, NaN, inf and 1e-22 (s*s is subnormal): the NaN and the inf
    make their records invalid, which every merge carries through as singletons, so they are nodes of every level"""
    rec = mr.crafted_records(n, seed)
    if n >= 65:
        for j, e in enumerate((0.0, np.nan, np.inf, 1e-22)):
            i = (n * (2 * j + 1)) // 9 + 1
            rec[i, 0:3] = (6.0 + j, -7.0, 5.0)
            rec[i, 8:10] = e
    return rec


def download_tree(conv):
    return conv.download_lod(0), conv.download_lod(1), conv.download_lod(2), conv.lod_levels()


def cameras(b, first):
    """far, between, inside a cluster, at a node's own position of the last level (d2 clamps to near^2)"""
    ok = np.flatnonzero(np.isfinite(b[:, 0:3]).all(1))
    leaf, top = ok[ok < first[1]], ok[ok >= first[-2]]
    mid = b[leaf[len(leaf) // 2], 0:3]
    return [(50.0, 40.0, 30.0), (3.0, 0.5, -2.0), tuple(float(v) for v in mid + F(0.02)), tuple(float(v) for v in b[top[0], 0:3])]


def check_budget(conv, ref, tree, parent, b, first, LH, cam, budget, tau_min, focal=FOCAL, near=NEAR):
    """one budget cut on `conv` against the restatement and, where `ref` holds the same tree, against lod_select at the returned tau_px"""
    L, H = LH
    want = br.search(L, H, first, budget, tau_min)
    sel = lr.select(b, parent, first, cam, focal, want["tau_px"], near)
    got = conv.lod_select_budget(cam, focal, budget, tau_min, near)
    print(f"lod budget nodes={first[-1]} cam={tuple(round(v, 3) for v in cam)} budget={budget} floor={tau_min}: {got} want key {want['key']:#x}")
    assert br.key_of(got["tau_px"]) == want["key"] and got["met"] == want["met"] and got["selected_finer"] == want["selected_finer"]
    assert got["selected"] == want["selected"] and got["per_level"] == sel["per_level"]
    assert {k: got[k] for k in lod.SELECT_COUNTS} == sel["counts"]
    ids = conv.download_lod_nodes()
    assert ids.dtype == np.uint32 and np.array_equal(ids, sel["nodes"]) and np.array_equal(ids, np.flatnonzero(br.flags_at(L, H, want["key"])))
    mine = bits(conv.download())
    assert conv.num_stored == len(ids) and np.array_equal(mine, bits(tree[ids]))
    if ref is not None:
        other = ref.lod_select(cam, focal, got["tau_px"], near)
        assert other == {k: got[k] for k in other}
        assert np.array_equal(ref.download_lod_nodes(), ids) and np.array_equal(bits(ref.download()), mine)
    SEEN["cuts"] += 1
    SEEN["mixed"] += sum(1 for v in sel["per_level"] if v) >= 2
    SEEN["unmet"] += not want["met"]
    SEEN["floor"] += want["by_floor"]
    SEEN["jump"] += want["key"] > 0 and not want["by_floor"] and want["selected"] < want["n_eff"] and want["selected_finer"] > want["n_eff"] + 1
    return got


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_budget_cuts_against_the_restatement_and_lod_select(conv, ref, n):
    rec = special_records(n, n)
    for levels in CHAINS:
        for max_group in (2, 64):
            for unsigned in (False, True):
                conv.upload_records(rec)
                out = conv.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned)
                ref.upload_records(rec)
                assert ref.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned) == out
                tree, parent, b, first = download_tree(conv)
                with np.errstate(all="ignore"):
                    SEEN["special_inner"] += int(np.count_nonzero(~np.isfinite(b[first[1]:, 3]) | (b[first[1]:, 3] < F(1e-20))))
                for cam in cameras(b, first):
                    L, H, _ = br.intervals(b, parent, first, cam, FOCAL, NEAR)
                    for budget in br.budgets(L, H, first):
                        for tau_min in (0.0, 2.0):
                            check_budget(conv, ref, tree, parent, b, first, (L, H), cam, budget, tau_min)


def test_grid_quadtree_budgets_on_the_device(conv):
    """the 8 x 8 grid quadtree from height 200, focal 512: the budgets return whole levels at the tau bits tests/test_lod_budget_ref.py derives"""
    conv.upload_records(mr.grid_records(8))
    assert conv.lod_build(levels=(8, 9, 10))["first"] == [0, 64, 80, 84, 85]
    tree, parent, b, first = download_tree(conv)
    cam = (0.5, 0.5, 200.0)
    LH = br.intervals(b, parent, first, cam, 512.0, 1.0)[:2]
    for budget, want, level, key, finer in ((64, 64, 0, 0, 64), (16, 16, 1, 0x3F23D707, 28), (4, 4, 2, 0x3FA3D6FA, 16), (1, 1, 3, 0x4023D70A, 4),
                                            (20, 16, 1, 0x3F23D707, 28)):
        got = check_budget(conv, None, tree, parent, b, first, LH, cam, budget, 0.0, 512.0, 1.0)
        assert got["per_level"] == [want if l == level else 0 for l in range(4)] and got["selected_finer"] == finer and got["met"]
        assert br.key_of(got["tau_px"]) == key


def test_ties_jump_across_the_budget(conv):
    """2 000 copies of one record in 500 places: the parents of one level share their bounds up to the place, and a camera far away sees
    whole groups of them change sides at one key"""
    rng = np.random.default_rng(3)
    base = mr.crafted_records(8, 0, invalid=False)[:1]
    rec = np.repeat(base, 2000, 0)
    rec[:, 8:10] = 0.05
    rec[:, 0:3] = np.repeat(rng.integers(-4, 5, (500, 3)).astype(F) / F(8), 4, 0)
    conv.upload_records(rec)
    out = conv.lod_build((0, 10), 64, -2.0)
    assert out["levels"] == 3 and out["first"][2] - 2000 <= 500
    tree, parent, b, first = download_tree(conv)
    cam = (0.0, 0.0, 4096.0)
    L, H, _ = br.intervals(b, parent, first, cam, FOCAL, NEAR)
    before = SEEN["jump"]
    for budget in sorted({1, 2, 700, 1500, 1999, 2000} | set(br.budgets(L, H, first))):
        check_budget(conv, None, tree, parent, b, first, (L, H), cam, budget, 0.0)
    assert SEEN["jump"] > before


def test_more_nodes_than_the_sweeps_lanes(conv, ref):
    """300 003 records, chain 1..10: more nodes than 1 024 x 256 lanes, levels of every size below, multi-workgroup histograms"""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    conv.upload_records(rec)
    out = conv.lod_build(tuple(range(1, 11)), 4, -2.0, unsigned_axis=True)
    ref.upload_records(rec)
    assert ref.lod_build(tuple(range(1, 11)), 4, -2.0, unsigned_axis=True) == out
    tree, parent, b, first = download_tree(conv)
    assert out["levels"] >= 4 and out["nodes"] > 1024 * 256
    mixed = 0
    for cam, budget, tau_min in (((0.3, -0.2, 0.1), 100000, 0.0), ((4.0, 3.0, 5.0), 20000, 0.0), ((4.0, 3.0, 5.0), 299999, 0.0), ((0.0, 0.0, 0.0), 50000, 1.0),
                                 ((4.0, 3.0, 5.0), 1, 0.0)):
        L, H, _ = br.intervals(b, parent, first, cam, FOCAL, NEAR)
        got = check_budget(conv, ref, tree, parent, b, first, (L, H), cam, budget, tau_min)
        mixed += sum(1 for v in got["per_level"] if v) >= 2
    assert mixed >= 2


def test_dry_run_changes_nothing_and_two_runs_give_the_same_bytes(conv):
    rec = special_records(300, 11)
    conv.upload_records(rec)
    conv.lod_build((3, 10), 4, 0.5)
    tree, parent, b, first = download_tree(conv)
    conv.upload_records(rec)                                                         # the tree survives other records
    conv.merge(2, 4, 0.5)
    rec2 = conv.download()
    sh = conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    conv.contrib_begin()
    conv.refit_begin()
    ptr, n2 = conv.device_records, conv.num_stored
    cam = (0.4, 0.1, -0.3)
    L, H, _ = br.intervals(b, parent, first, cam, FOCAL, NEAR)
    budget = (first[-1] - first[-2] + br.count(L, H, 0)) // 2
    want = br.search(L, H, first, budget)
    sel = lr.select(b, parent, first, cam, FOCAL, want["tau_px"], NEAR)
    dry = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, dry_run=True)
    assert br.key_of(dry["tau_px"]) == want["key"] and dry["met"] and dry["selected_finer"] == want["selected_finer"] > budget >= dry["selected"]
    assert dry["per_level"] == sel["per_level"] and {k: dry[k] for k in lod.SELECT_COUNTS} == sel["counts"]
    assert conv.device_records == ptr and conv.num_stored == n2 and np.array_equal(bits(conv.download()), bits(rec2))
    assert conv.device_contrib(0) and conv.device_refit(0) and conv.device_sh and conv.device_merge_map and conv.device_lod_nodes == 0
    assert np.array_equal(bits(conv.download_sh()), bits(sh))
    with pytest.raises(M2SError):
        conv.download_lod_nodes()
    real = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR)
    assert real == dry and conv.num_stored == want["selected"]
    assert conv.device_contrib(0) == 0 and conv.device_refit(0) == 0 and conv.device_sh == 0 and conv.device_merge_map == 0
    assert not conv.positions_ready and conv.device_lod_nodes != 0
    ids, out = conv.download_lod_nodes(), bits(conv.download()).copy()
    assert np.array_equal(ids, sel["nodes"]) and np.array_equal(out, bits(tree[ids]))
    assert conv.lod_select_budget(cam, FOCAL, budget, near=NEAR) == real             # again: the same result and bytes
    assert np.array_equal(conv.download_lod_nodes(), ids) and np.array_equal(bits(conv.download()), out)
    for x, y in zip(download_tree(conv)[:3], (tree, parent, b)):                     # the tree is untouched
        assert np.array_equal(bits(x), bits(y))
    ms = conv.last_lod_budget_stage_ms
    assert set(ms) == {"thresholds", "select", "cut"}


def test_stage_times_with_profiling(conv):
    conv.upload_records(special_records(4099, 2))
    conv.lod_build((3, 10), 4, 0.5)
    conv.set_profiling(True)
    try:
        conv.lod_select_budget((3.0, 0.5, -2.0), FOCAL, 1000, near=NEAR)
        ms, cut = conv.last_lod_budget_stage_ms, conv.last_lod_select_stage_ms()
        print(f"lod budget stages, 4 099 leaves: {ms}")
        assert ms["thresholds"] > 0 and ms["select"] > 0 and ms["cut"] == float(F(F(F(cut["sweep"]) + F(cut["scan_ids"])) + F(cut["compact"])))
    finally:
        conv.set_profiling(False)


def test_the_quads_conversion_in_world_units_returns_whole_levels(conv):
    """the unit quad at R = 64, in world units, unsigned tree: 4 096 / 1 024 / 256 / 64 / 16 / 4 / 1 nodes per level.  From (0.5, 0.5, 2)
    the distances within a level differ by 6 % at most and the edges of neighbouring levels by a factor of 2, so the cut passes through
    every whole level, and a budget of a level's size returns that level"""
    conv.upload_scene(synth.unit_quad())
    assert conv.convert(64) == 4096
    conv.to_world_units()
    out = conv.lod_build((4, 5, 6, 7, 8, 9, 10), 4, 0.5, unsigned_axis=True)
    assert list(np.diff(out["first"])) == [4096, 1024, 256, 64, 16, 4, 1]
    tree, parent, b, first = download_tree(conv)
    cam = (0.5, 0.5, 2.0)
    LH = br.intervals(b, parent, first, cam, 154.51, 1e-3)[:2]
    last_tau = -1.0
    for level, budget in enumerate((4096, 1024, 256, 64)):
        got = check_budget(conv, None, tree, parent, b, first, LH, cam, budget, 0.0, 154.51, 1e-3)
        assert got["per_level"] == [budget if l == level else 0 for l in range(7)] and got["met"] and got["tau_px"] > last_tau
        last_tau = got["tau_px"]
    assert check_budget(conv, None, tree, parent, b, first, LH, cam, 1023, 0.0, 154.51, 1e-3)["selected"] <= 1023


def test_adopted_memory_is_not_written_and_the_leaves_resolution_is_kept(conv, hiplib):
    rec = mr.crafted_records(1000, 13)
    owner = Converter(0)
    try:
        owner.upload_records(rec)
        conv.set_records(owner.device_records, len(rec), 48)
        assert conv.lod_build((2, 5, 10), 4, 0.5)["levels"] > 1
        tree, parent, b, first = download_tree(conv)
        conv.set_records(owner.device_records, len(rec), 99)                         # other current records, another resolutionTarget
        cam = (0.2, 0.2, 0.2)
        LH = br.intervals(b, parent, first, cam, FOCAL, NEAR)[:2]
        check_budget(conv, None, tree, parent, b, first, LH, cam, 400, 0.0)
        assert conv.device_records != owner.device_records and hiplib.m2s_last_resolution(conv._h) == 48
        assert np.array_equal(bits(owner.download()), bits(rec))
    finally:
        owner.close()


def test_errors_the_empty_tree_and_release(hiplib):
    c = Converter(0)
    try:
        out = (C.c_uint64 * 4)()
        res = lod.LodBudgetResultC()

        def select(cam=(0.0, 0.0, 0.0), focal=500.0, budget=10, tau_min=0.0, near=0.1, flags=0):
            p = lod.budget_to_c(cam, focal, budget, tau_min, near)
            p.flags = flags
            return hiplib.m2s_lod_select_budget(c._h, C.byref(p), C.byref(res), out)

        assert select() == 7                                                         # no tree
        rec = mr.crafted_records(40, 1)
        c.upload_records(rec)
        c.lod_build((3, 10), 4, 0.5)
        nan, inf = float("nan"), float("inf")
        for bad in (dict(cam=(nan, 0, 0)), dict(cam=(0, inf, 0)), dict(cam=(0, 0, -inf)), dict(focal=0.0), dict(focal=-1.0), dict(focal=nan), dict(focal=inf),
                    dict(tau_min=-1.0), dict(tau_min=nan), dict(tau_min=inf), dict(near=0.0), dict(near=-1.0), dict(near=nan), dict(near=inf), dict(flags=2),
                    dict(flags=3), dict(budget=0)):
            assert select(**bad) == 1, bad
        assert hiplib.m2s_lod_select_budget(c._h, None, None, None) == 1
        before = c.download()
        assert select(flags=1) == 0 and np.array_equal(bits(c.download()), bits(before))
        p = lod.budget_to_c((0.0, 0.0, 0.0), 500.0, 10, near=0.1)
        assert hiplib.m2s_lod_select_budget(c._h, C.byref(p), None, None) == 0                           # (both outputs may be NULL)
        assert c.num_stored == c.lod_select_budget((0.0, 0.0, 0.0), 500.0, 10, near=0.1, dry_run=True)["selected"] < 40
        # zero records build an empty tree: the floor, met, nothing selected
        c.upload_records(np.zeros((0, 24), F))
        c.lod_build((1,))
        got = c.lod_select_budget((0, 0, 0), 500.0, 5, tau_min_px=2.0)
        assert got == {"nodes": 0, "selected": 0, "selected_leaves": 0, "refine": 0, "per_level": [0], "tau_px": 2.0, "met": True, "selected_finer": 0}
        assert c.lod_select_budget((0, 0, 0), 500.0, 5)["tau_px"] == 0.0 and c.num_stored == 0
        # conversions in flight: refused, the conversion still delivered
        c.upload_records(rec)
        c.lod_build((3, 10), 4, 0.5)
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()
        c.submit(48)
        assert select() == 7 and select(flags=1) == 7 and b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total
        assert select() == 0
        c.lod_release()
        assert select() == 7 and select(flags=1) == 7
    finally:
        c.close()


def test_zz_the_cases_exercise_mixed_unmet_floor_and_jumps():
    """Runs last in this module: over the cuts above some took nodes of two levels or more, some budgets lay below the last level, some
    results were decided by the floor, some counts jumped across the budget, and nodes above the leaves had the special edges."""
    print(f"lod budget, over the module: {SEEN}")
    assert SEEN["cuts"] > 1000 and all(v > 0 for v in SEEN.values()), SEEN
