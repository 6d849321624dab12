"""CPU: the symbols, the struct layout and the NULL handling of m2s_prune_budget / m2s_upload_contrib (no compute calls), and the numpy
restatement of the pin (tests/budget_ref.py): its two selections against each other on every key family, the keys' monotonicity."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import budget_cases as bc
import budget_ref as br
from mesh2splat_amd import _lib
from mesh2splat_amd.prune import BUDGET_COUNTS, IMPORTANCE, BudgetParamsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2s_prune_budget", "m2s_last_budget_counts", "m2s_last_budget_stage_ms", "m2s_upload_contrib")


def test_symbols_exported(hiplib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(hiplib, name), name


def test_ctypes_mirror_layout():
    assert C.sizeof(BudgetParamsC) == 24 and [getattr(BudgetParamsC, f).offset for f, _ in BudgetParamsC._fields_] == [0, 8, 12, 16, 20]
    assert IMPORTANCE == {"views": 0, "area": 1} and BUDGET_COUNTS == br.COUNTS


def test_struct_layout_matches_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    fields = ("max_records", "min_weight", "min_pixels", "importance", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){printf("%zu ' + "%zu " * len(fields) + '%d %d\\n", '
                   "sizeof(m2s_budget_params), " + ", ".join(f"offsetof(m2s_budget_params, {f})" for f in fields) +
                   ", (int)M2S_IMPORTANCE_VIEWS, (int)M2S_IMPORTANCE_AREA);return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(BudgetParamsC)] + [getattr(BudgetParamsC, f).offset for f in fields] + [0, 1] and out[0] == 24


def test_null_context(hiplib):
    bp = BudgetParamsC(1, 0.0, 0, 0, 0)
    kept, out6, out3, words = C.c_uint64(), (C.c_uint64 * 6)(), (C.c_float * 3)(), (C.c_uint32 * 1)()
    assert hiplib.m2s_prune_budget(None, C.byref(bp), C.byref(kept)) == 1
    assert hiplib.m2s_last_budget_counts(None, out6) == 1 and hiplib.m2s_last_budget_stage_ms(None, out3) == 1
    assert hiplib.m2s_upload_contrib(None, words, words, 1) == 1


def _check_selection(keys, cand, B):
    kept, counts = br.select(keys, cand, B)
    assert np.array_equal(kept, br.select_by_sort(keys, cand, B))
    nc = int(np.count_nonzero(cand))
    assert counts["before"] == keys.size and counts["candidates"] == nc and counts["kept"] == kept.size == min(B, nc)
    assert cand[kept].all() and np.all(np.diff(kept) > 0)
    if nc > B:
        T = counts["threshold_key"]
        ck = keys[cand]
        assert counts["ties"] == int((ck == T).sum()) and counts["ties_kept"] == B - int((ck > T).sum()) and 1 <= counts["ties_kept"] <= counts["ties"]
        assert keys[kept].min() == T and (keys[np.setdiff1d(np.flatnonzero(cand), kept)] <= T).all()
    else:
        assert (counts["threshold_key"], counts["ties_kept"], counts["ties"]) == (0, 0, 0)


@pytest.mark.parametrize("name", bc.FAMILIES)
def test_the_two_restatements_agree(name):
    for n in bc.SIZES:
        w, k = bc.family(name, n)
        keys = br.keys_views(w, k)
        for B in bc.budgets(n):
            _check_selection(keys, br.candidates_views(w, k, -1.0, 0), B)
            # ... and with thresholds that bind
            _check_selection(keys, br.candidates_views(w, k, np.median(w.view(np.float32)), 3), max(1, B // 2))


def test_family_keys_are_what_they_claim():
    w, k = bc.family("all_equal", 257)
    assert np.unique(br.keys_views(w, k)).size == 1
    for d in range(3):
        w, k = bc.family(f"digit{d}", 1000)
        keys = br.keys_views(w, k)
        assert np.array_equal(keys, w) and np.unique(keys & ~np.uint32(0xFF << (8 * d))).size == 1 and np.unique(keys).size > 64
    w, k = bc.family("digit3", 1000)
    assert np.array_equal(br.keys_views(w, k), w) and set(np.unique(w >> 24)) == {0x00, 0x10, 0x20, 0x3F} and not (w & 0xFFFFFF).any()
    w, k = bc.family("half_zero", 1000)
    assert 350 < (br.keys_views(w, k) == 0).sum() < 650


def test_views_key_is_monotone():
    rng = np.random.default_rng(3)
    w = np.sort(rng.integers(0, bc.ONE + 1, 20000, dtype=np.uint32))
    for npix in (0, 1, 3, 50, 1 << 24, (1 << 24) + 1, (1 << 30) - 1):
        keys = br.keys_views(w, np.full(w.size, npix, np.uint32))
        assert np.all(np.diff(keys.astype(np.int64)) >= 0) and keys.max() < 0x7F800000
    k = np.sort(rng.integers(0, 1 << 30, 20000, dtype=np.uint32))
    for wb in (0, 1, 0x00800000, 0x3C000000, 0x3F7FFFFF, bc.ONE):
        keys = br.keys_views(np.full(k.size, wb, np.uint32), k)
        assert np.all(np.diff(keys.astype(np.int64)) >= 0)


def test_area_keys_of_planted_records():
    rec = bc.planted_area_records()
    keys = br.keys_area(rec)
    INF = 0x7F800000
    assert keys.max() == INF and keys[40] == INF and keys[41] == INF and keys[90] == INF
    for i in (3, 10, 30, 51, 52, 60, 61, 70, 71, 80):
        assert keys[i] == 0, i
    assert 0 < keys[81] < 0x00800000                                            # a denormal product keeps its bits
    assert keys[20] == np.float32(np.float32(2.5) * np.abs(rec[20, 9]) * rec[20, 7]).view(np.uint32)
    assert keys[21] == np.float32(np.float32(12.0) * rec[21, 7]).view(np.uint32) and keys[50] == np.float32(rec[50, 8] * rec[50, 9]).view(np.uint32)
    _check_selection(keys, np.ones(keys.size, bool), 100)
