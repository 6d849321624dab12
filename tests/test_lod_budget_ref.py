"""CPU: the restatement of the cut that fits a budget (tests/lod_budget_ref.py) held to the restatement of the cut itself
(tests/lod_ref.py): the interval rule gives lod_ref.select's flags at every key where anything changes, the count never increases with
the key, and the search returns the smallest key that fits.  Then cases derived by hand, the structs against the C compiler's layout,
the symbols and the entry points' NULL checks (no device needed)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import lod_budget_ref as br
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def random_tree(rng, k):
    """sizes that go up and down along a chain; nodes with e = 0, NaN, inf and 1e-22 (s*s is subnormal), one NaN position, and in every
    fourth tree a node at the camera with a `near` whose square is 0"""
    levels = int(rng.integers(2, 7))
    counts = [int(rng.integers(12, 40))]
    for _ in range(levels - 1):
        counts.append(max(1, int(counts[-1] * rng.uniform(0.3, 0.9))))
    maps = [np.sort(np.concatenate([np.arange(counts[l + 1]), rng.integers(0, counts[l + 1], counts[l] - counts[l + 1])])).astype(np.uint32)
            for l in range(levels - 1)]
    parent, first = lr.link(maps, counts)
    n = first[-1]
    b = np.empty((n, 4), F)
    b[:, 0:3] = rng.normal(0, 1, (n, 3))
    b[:, 3] = np.exp(rng.normal(-2, 1.5, n)) * (rng.random(n) > 0.1)
    inner = np.arange(first[1], n)
    for e in (0.0, np.nan, np.inf, 1e-22):
        b[rng.choice(inner), 3] = e
    b[rng.choice(inner), 0] = np.nan
    cam = tuple(float(F(v)) for v in rng.normal(0, 2, 3))
    near = 0.05
    if k % 4 == 0:
        near = 1e-30                                                                 # near * near == 0 in float32
        b[rng.choice(inner), 0:3] = cam                                              # d2 == 0
        assert F(near) * F(near) == 0
    return b, parent, first, cam, float(rng.uniform(50, 2000)), near


def test_interval_rule_is_the_cut_and_the_search_is_tight_on_random_trees():
    rng = np.random.default_rng(23)
    seen = {"mixed": 0, "unmet": 0, "floor": 0, "jump": 0, "empty_interval": 0}
    for k in range(200):
        b, parent, first, cam, focal, near = random_tree(rng, k)
        L, H, T = br.intervals(b, parent, first, cam, focal, near)
        assert T.max() <= br.KEY_MAX and (H[first[-2]:] == br.NEVER).all() and (L[:first[1]] == 0).all()
        seen["empty_interval"] += int(np.count_nonzero(L >= H))
        ends = br.endpoints(L, H)
        prev = None
        for e in ends:
            for key in ((e - 1, e) if e else (e,)):
                sel = lr.select(b, parent, first, cam, focal, br.tau_of(key), near)
                assert np.array_equal(br.flags_at(L, H, key), sel["flags"]), (k, key)
                c = br.count(L, H, key)
                assert c == sel["counts"]["selected"] and (prev is None or c <= prev)
                prev = c
        last = first[-1] - first[-2]
        assert br.count(L, H, br.KEY_MAX) == last and br.count(L, H, 0) == lr.select(b, parent, first, cam, focal, 0.0, near)["counts"]["selected"]
        for budget in br.budgets(L, H, first):
            got = br.search(L, H, first, budget)
            n_eff = max(budget, last)
            assert got["n_eff"] == n_eff and got["selected"] == br.count(L, H, got["key"]) <= n_eff
            assert got["key"] == 0 or br.count(L, H, got["key"] - 1) > n_eff
            assert got["met"] == (got["selected"] <= budget) and got["met"] == (budget >= last)
            assert got["selected_finer"] == (got["selected"] if got["key"] == 0 else br.count(L, H, got["key"] - 1))
            sel = lr.select(b, parent, first, cam, focal, got["tau_px"], near)
            assert sel["counts"]["selected"] == got["selected"] and lr.cut_ok(parent, first, sel["flags"])
            seen["mixed"] += sum(1 for v in sel["per_level"] if v) >= 2
            seen["unmet"] += not got["met"]
            seen["jump"] += got["key"] > 0 and got["selected"] < n_eff and got["selected_finer"] > n_eff + 1
            # the floor wins where it is larger, and only there
            for tau_min in (br.tau_of(max(got["key"] - 1, 0)), br.tau_of(got["key"]), br.tau_of(got["key"] + 1000), F(3.0)):
                fl = br.search(L, H, first, budget, tau_min)
                fk = br.key_of(tau_min)
                assert fl["key"] == max(got["key"], fk) and fl["by_floor"] == (fk > got["key"])
                assert fl["selected"] == br.count(L, H, fl["key"]) <= got["selected"]
                assert fl["selected_finer"] == (fl["selected"] if fl["by_floor"] or fl["key"] == 0 else got["selected_finer"])
                seen["floor"] += fl["by_floor"]
    print(f"lod budget restatement, over 200 trees: {seen}")
    assert all(v > 0 for v in seen.values()), seen


@pytest.fixture(scope="module")
def grid_tree():
    """merge_ref.grid_records(8) through merges at levels 8, 9, 10: a perfect quadtree of 64 / 16 / 4 / 1 nodes, edges 0.125 .. 1.0"""
    levels, maps = [mr.grid_records(8)], []
    for lv in (8, 9, 10):
        out, mp, _, _ = mr.merge(levels[-1], lv, 4, 0.5)
        levels.append(out)
        maps.append(mp)
    counts = [len(v) for v in levels]
    assert counts == [64, 16, 4, 1]
    parent, first = lr.link(maps, counts)
    return lr.bounds(np.concatenate(levels)), parent, first


def smallest_tau_bits(ss, d2):
    """the bits of the smallest float32 tau with fl(fl(tau * tau) * d2) >= ss, by scalar arithmetic of its own: the square of a float32 and
    the product of two are exact in float64, so rounding them to float32 is the one rounding the pin asks for"""
    def holds(t):
        return float(F(float(F(float(t) * float(t))) * d2)) >= ss
    t = F(math.sqrt(ss / d2))
    while holds(t):
        t = np.nextafter(t, F(0))
    while not holds(t):
        t = np.nextafter(t, F(np.inf))
    return br.key_of(t)


# Camera (0.5, 0.5, 200), focal 512, near 1.  A node of level l has e = 2^l / 8, s = 64 * 2^l, s*s = 4096 * 4^l, all exact.  The root is at
# d2 = 200^2 = 40000; the four nodes of level 2 at dx, dy = +-0.25: d2 = 40000.125; of the sixteen of level 1 the four in the middle
# (dx, dy = +-0.125) are nearest, d2 = 40000.03125.  tau*tau*d2 >= s*s first holds near tau = sqrt(s*s / d2) = 2.56, 1.28, 0.64:
GRID_KEYS = {1: 0x4023D70A, 4: 0x3FA3D6FA, 16: 0x3F23D707}


def test_grid_quadtree_budgets_return_whole_levels(grid_tree):
    b, parent, first = grid_tree
    cam, focal, near = (0.5, 0.5, 200.0), 512.0, 1.0
    L, H, T = br.intervals(b, parent, first, cam, focal, near)
    assert GRID_KEYS == {1: smallest_tau_bits(262144.0, 40000.0), 4: smallest_tau_bits(65536.0, 40000.125), 16: smallest_tau_bits(16384.0, 40000.03125)}
    assert int(T[first[3]]) == GRID_KEYS[1] and (T[first[2]:first[3]] == GRID_KEYS[4]).all() and int(T[first[1]:first[2]].max()) == GRID_KEYS[16]
    for budget, want, level, key in ((64, 64, 0, 0), (16, 16, 1, GRID_KEYS[16]), (4, 4, 2, GRID_KEYS[4]), (1, 1, 3, GRID_KEYS[1]), (20, 16, 1, GRID_KEYS[16]),
                                     (63, 52, None, None), (1000, 64, 0, 0)):
        got = br.search(L, H, first, budget)
        sel = lr.select(b, parent, first, cam, focal, got["tau_px"], near)
        assert got["selected"] == want == sel["counts"]["selected"] and got["met"]
        if level is not None:
            assert got["key"] == key and sel["per_level"] == [want if l == level else 0 for l in range(4)]
    # the mixed cuts that do exist: the level-1 nodes lie at three distances (4, 8 and 4 of them), so the count steps 16 -> 28 -> 52 -> 64
    assert sorted({br.count(L, H, k) for k in br.endpoints(L, H)}) == [1, 4, 16, 28, 52, 64]
    assert br.search(L, H, first, 20)["selected_finer"] == 28


def test_ties_jump_across_the_budget_to_the_coarser_side():
    """40 leaves under 10 parents with one and the same bound under one root: every parent has the same T, so the count is 40, 10 or 1 and
    nothing between: a budget of 25 gets 10"""
    maps = [np.repeat(np.arange(10, dtype=np.uint32), 4), np.zeros(10, np.uint32)]
    parent, first = lr.link(maps, [40, 10, 1])
    b = np.zeros((51, 4), F)
    b[:, 0:3] = (1.0, 2.0, 3.0)
    b[:40, 3], b[40:50, 3], b[50, 3] = 0.01, 0.1, 0.5
    cam, focal, near = (0.0, 0.0, 0.0), 700.0, 0.1
    L, H, T = br.intervals(b, parent, first, cam, focal, near)
    assert len(set(T[40:50].tolist())) == 1 and T[40] < T[50]
    for budget, want, finer in ((40, 40, 40), (39, 10, 40), (25, 10, 40), (10, 10, 40), (9, 1, 10), (1, 1, 10)):
        got = br.search(L, H, first, budget)
        assert (got["selected"], got["selected_finer"], got["met"]) == (want, finer, True), (budget, got)
    assert br.search(L, H, first, 25)["key"] == int(T[40]) and br.search(L, H, first, 9)["key"] == int(T[50])


def test_an_empty_tree_gives_the_floor():
    L = H = np.zeros(0, np.uint32)
    got = br.search(L, H, [0, 0], 5, 2.0)
    assert got["tau_px"] == F(2.0) and got["met"] and got["selected"] == 0 and got["selected_finer"] == 0
    assert br.search(L, H, [0, 0], 5)["key"] == 0


def test_struct_layouts_match_the_header(tmp_path):
    assert C.sizeof(lod.LodBudgetParamsC) == 32 and C.sizeof(lod.LodBudgetResultC) == 16
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = {"m2s_lod_budget_params": [f[0] for f in lod.LodBudgetParamsC._fields_], "m2s_lod_budget_result": [f[0] for f in lod.LodBudgetResultC._fields_]}
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu %zu\\n", sizeof(m2s_lod_budget_params), sizeof(m2s_lod_budget_result));\n' +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (s, f) for s, fs in fields.items() for f in fs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[:2]] == [32, 16]
    want = [getattr(lod.LodBudgetParamsC, f).offset for f in fields["m2s_lod_budget_params"]] + \
           [getattr(lod.LodBudgetResultC, f).offset for f in fields["m2s_lod_budget_result"]]
    assert [int(v) for v in out[2:]] == want == [0, 12, 16, 20, 24, 28, 0, 4, 8]


def test_budget_to_c():
    p = lod.budget_to_c((1, 2, 3), 500.0, 7, tau_min_px=0.5, near=0.25, dry_run=True)
    assert (list(p.camera_position), p.focal_px, p.near, p.tau_min_px, p.max_records, p.flags) == ([1.0, 2.0, 3.0], 500.0, 0.25, 0.5, 7, lod.DRY_RUN)
    assert lod.budget_to_c((0, 0, 0), 1.0, 0xFFFFFFFF).flags == 0
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            lod.budget_to_c((0, 0, 0), 1.0, bad)


def test_symbols_and_null_contexts(hiplib):
    assert hiplib.m2s_lod_select_budget and hiplib.m2s_last_lod_budget_stage_ms
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    res = lod.LodBudgetResultC(3.0, 9, 9)
    p = lod.budget_to_c((0, 0, 0), 500.0, 10)
    assert hiplib.m2s_lod_select_budget(None, C.byref(p), C.byref(res), out) == 1
    assert list(out) == [0, 0, 0, 0] and (res.tau_px, res.met, res.selected_finer) == (0.0, 0, 0)
    assert hiplib.m2s_lod_select_budget(None, None, None, None) == 1
    ms = (C.c_float * 3)()
    assert hiplib.m2s_last_lod_budget_stage_ms(None, ms) == 1
