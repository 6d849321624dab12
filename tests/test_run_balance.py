"""The dispatch order of the runs (launch_run_order): run_balance_assign (mesh2splat_amd/csrc/m2s_run_balance.h) deals the runs, sorted by
weight, to the eight XCD queues (dispatch slot s belongs to XCD s % 8).  No GPU: the header is compiled into a stand-alone host program
(tests/run_balance/run_balance_check.cpp) with -fsanitize=address,undefined, and that program — the device's code — is run once on every
case below.

Weights: config 3's 3916 per-unit fragment counts (tests/golden/run_balance_c3_units.npy, written by tools/xcd_balance.py from the CPU
oracle; sum 2 738 368) in runs of 32 and of 16 units; a strictly descending ramp, all-equal weights and a single heavy run, each at every
n_runs from 1 to 40 (every n_runs % 8, queues of unequal length).

Asserted for every case: order[] over the slots that hold a run is a permutation of the ranks; padding slots hold themselves; every queue
is non-increasing in weight.  On config 3 at 32-unit runs the heaviest queue holds at most 1.025 x the mean (the assignment gives 1.0212;
rank r in slot r, shipped before, gives 1.0506 and must fail that bound)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import xcd_balance  # noqa: E402

C3_SUM = 2738368


def c3_units():
    u = np.load(os.path.join(ROOT, "tests", "golden", "run_balance_c3_units.npy")).astype(np.int64)
    assert len(u) == 3916 and int(u.sum()) == C3_SUM
    return u


def weight_sets():
    """name -> costs in RUN order (any order); the test ranks them as k_run_rank does"""
    sets = {}
    u = c3_units()
    sets["c3/32"] = xcd_balance.run_costs(u, 5)
    sets["c3/16"] = xcd_balance.run_costs(u, 4)
    for n in range(1, 41):
        sets[f"ramp/{n}"] = np.arange(n, 0, -1, dtype=np.int64) * 1000 + 7
        sets[f"equal/{n}"] = np.full(n, 22263, np.int64)
        heavy = np.full(n, 100, np.int64)
        heavy[n // 2] = 1000000
        sets[f"heavy/{n}"] = heavy
    return sets


@pytest.fixture(scope="module")
def assigned(tmp_path_factory):
    """name -> (costs in rank order, order[] of the compiled header)"""
    cxx = next((p for p in (shutil.which(n) for n in ("c++", "g++", "clang++")) if p), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("run_balance") / "run_balance_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "mesh2splat_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "run_balance", "run_balance_check.cpp")],
                   check=True)
    sets = weight_sets()
    ranked, lines = {}, []
    for name, costs in sets.items():
        by_rank = costs[xcd_balance.ranked(costs)]
        n_slots = (len(by_rank) + 7) // 8 * 8
        ranked[name] = by_rank
        lines.append(" ".join(map(str, [len(by_rank), n_slots] + by_rank.tolist())))
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    rows = done.stdout.strip().split("\n")
    assert len(rows) == len(sets)
    return {name: (ranked[name], np.array(row.split(), np.int64)) for name, row in zip(sets, rows)}


def test_cases_cover_every_remainder(assigned):
    assert {len(by_rank) % 8 for by_rank, _ in assigned.values()} == set(range(8))
    assert len(assigned["c3/32"][0]) == 123 and len(assigned["c3/16"][0]) == 245


def test_permutation_and_padding(assigned):
    for name, (by_rank, order) in assigned.items():
        n = len(by_rank)
        assert len(order) == (n + 7) // 8 * 8, name
        assert sorted(order[:n].tolist()) == list(range(n)), name
        assert order[n:].tolist() == list(range(n, len(order))), name


def test_every_queue_is_heaviest_first(assigned):
    for name, (by_rank, order) in assigned.items():
        n = len(by_rank)
        for x in range(8):
            ranks = order[x::8]
            w = by_rank[ranks[ranks < n]]
            assert np.all(np.diff(w) <= 0), (name, x, w.tolist())


def test_c3_queues_hold_equal_work(assigned):
    by_rank, order = assigned["c3/32"]
    q = xcd_balance.queue_sums(order, by_rank)
    print("config 3, runs of 32 units: queue sums", q.tolist(), "heaviest / mean", q.max() / q.mean())
    assert int(q.sum()) == C3_SUM
    assert q.max() <= 1.025 * q.mean()
    by_rank16, order16 = assigned["c3/16"]
    q16 = xcd_balance.queue_sums(order16, by_rank16)
    print("config 3, runs of 16 units (not shipped): queue sums", q16.tolist(), "heaviest / mean", q16.max() / q16.mean())
    assert int(q16.sum()) == C3_SUM


def test_rank_to_slot_misses_the_bound():
    """the premise: the order shipped before (rank r in slot r) leaves config 3's heaviest queue 5 % above the mean"""
    costs = xcd_balance.run_costs(c3_units(), 5)
    by_rank = costs[xcd_balance.ranked(costs)]
    q = xcd_balance.queue_sums(xcd_balance.assign_rank_to_slot(by_rank, 128), by_rank)
    assert q.max() > 1.025 * q.mean() and abs(q.max() / q.mean() - 1.0506) < 1e-4


def test_single_heavy_run_stands_alone(assigned):
    """the queue that got the heavy run takes nothing more while another queue has a free slot: the rest of its slots (every queue ends
    full) hold the last ranks"""
    for n in range(9, 41):
        by_rank, order = assigned[f"heavy/{n}"]
        x = int(np.flatnonzero(order[:8] == 0)[0])
        ranks = order[x::8]
        ranks = ranks[ranks < n]
        assert ranks.tolist() == [0] + list(range(n - (len(ranks) - 1), n)), (n, ranks.tolist())


def test_tool_mirrors_the_header(assigned):
    for name, (by_rank, order) in assigned.items():
        assert np.array_equal(xcd_balance.assign_balanced(by_rank, len(order)), order), name
