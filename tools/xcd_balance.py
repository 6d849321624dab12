"""How evenly a dispatch order of the runs spreads a scene's fragments over the eight XCD queues (RunInfo, m2s_device.h; the shipped
assignment is run_balance_assign, mesh2splat_amd/csrc/m2s_run_balance.h, mirrored here line by line).  No GPU needed.

Input: per-triangle fragment counts — a .npy written from Converter.download_triangle_counts(), the per-unit fixture of the tests, or the
CPU oracle's count of a cube-sphere scene.  Output: for each run length asked for, one line per assignment with the heaviest queue over
the mean, (heaviest - lightest) over the mean and the eight sums.

    python tools/xcd_balance.py --oracle 289 1024                    # config 3 (about 50 s of CPU), runs of 32 and 16 units
    python tools/xcd_balance.py --counts counts.npy --unit 512 --shifts 5
    python tools/xcd_balance.py --units tests/golden/run_balance_c3_units.npy
    python tools/xcd_balance.py --oracle 289 1024 --write-units tests/golden/run_balance_c3_units.npy   # regenerates the fixture
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
QUEUES = 8


def run_costs(units, shift):
    """fragments per run of (1 << shift) consecutive units"""
    units = np.asarray(units, np.int64)
    return np.add.reduceat(units, np.arange(0, len(units), 1 << shift))


def ranked(costs):
    """run ids, heaviest first (ties: lower run first) — k_run_rank"""
    return np.argsort(-np.asarray(costs, np.int64), kind="stable")


def assign_balanced(cost_by_rank, n_slots):
    """run_balance_assign: order[slot] = rank"""
    n = len(cost_by_rank)
    order = np.arange(n_slots, dtype=np.int64)
    load, used = [0] * QUEUES, [0] * QUEUES
    cap = [(n - x + QUEUES - 1) // QUEUES if n > x else 0 for x in range(QUEUES)]
    for r in range(n):
        best = None
        for x in range(QUEUES - 1, -1, -1):
            if used[x] < cap[x] and (best is None or (load[x], used[x]) < (load[best], used[best])):
                best = x
        order[used[best] * QUEUES + best] = r
        load[best] += int(cost_by_rank[r])
        used[best] += 1
    return order


def assign_rank_to_slot(cost_by_rank, n_slots):
    """rank r in slot r (shipped from round 7 to round 11)"""
    return np.arange(n_slots, dtype=np.int64)


def assign_boustrophedon(cost_by_rank, n_slots):
    """sorted, odd groups of eight reversed"""
    n = len(cost_by_rank)
    order = np.arange(n_slots, dtype=np.int64)
    full = (n // QUEUES) * QUEUES
    g = order[:full].reshape(-1, QUEUES)
    g[1::2] = g[1::2, ::-1].copy()
    return order


def queue_sums(order, cost_by_slot_value):
    """fragments per XCD queue of an order whose entries index cost_by_slot_value (entries past its end: padding)"""
    w = np.zeros(len(order), np.int64)
    real = order < len(cost_by_slot_value)
    w[real] = np.asarray(cost_by_slot_value, np.int64)[order[real]]
    return w.reshape(-1, QUEUES).sum(axis=0)


def table(units, shift):
    costs = run_costs(units, shift)
    n = len(costs)
    n_slots = (n + QUEUES - 1) // QUEUES * QUEUES
    by_rank = costs[ranked(costs)]
    rows = [("mesh order", queue_sums(np.arange(n_slots), costs)),
            ("sorted, rank r to slot r", queue_sums(assign_rank_to_slot(by_rank, n_slots), by_rank)),
            ("sorted, boustrophedon", queue_sums(assign_boustrophedon(by_rank, n_slots), by_rank)),
            ("sorted, least-loaded queue with a free slot (shipped)", queue_sums(assign_balanced(by_rank, n_slots), by_rank))]
    print(f"runs of {1 << shift} units: {n} runs holding {costs.min()} ... {costs.max()} fragments, {costs.sum()} in all, mean queue {costs.sum() / QUEUES:.0f}")
    for name, q in rows:
        print(f"  {name:55s} heaviest / mean {q.max() / q.mean():.4f}  (heaviest - lightest) / mean {100.0 * (q.max() - q.min()) / q.mean():5.2f} %  {q.tolist()}")
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--counts", help=".npy of per-triangle fragment counts")
    src.add_argument("--units", help=".npy of per-unit fragment counts (unit as in --unit)")
    src.add_argument("--oracle", nargs=2, type=int, metavar=("N", "R"), help="count cube_sphere(N) at density R with the CPU oracle")
    ap.add_argument("--unit", type=int, default=256, help="triangles per unit: 256 (k_fused2 / k_fused3) or 512 (k_sparse)")
    ap.add_argument("--shifts", type=int, nargs="+", default=[5, 4], help="log2 of the run lengths to tabulate")
    ap.add_argument("--write-units", help="store the per-unit counts (uint32 .npy) here")
    a = ap.parse_args()
    if a.units:
        units = np.load(a.units).astype(np.int64)
    else:
        if a.counts:
            cnt = np.load(a.counts).astype(np.int64)
        else:
            sys.path.insert(0, ROOT)
            from mesh2splat_amd import synth
            from oracle import oracle
            cnt = oracle.count_per_triangle(synth.colocated_spheres(1, a.oracle[0], 0), a.oracle[1]).astype(np.int64)
        units = np.add.reduceat(cnt, np.arange(0, len(cnt), a.unit))
    print(f"{len(units)} units of {a.unit} triangles holding {units.min()} ... {units.max()} fragments, sum {units.sum()}")
    if a.write_units:
        np.save(a.write_units, units.astype(np.uint32))
    for shift in a.shifts:
        table(units, shift)


if __name__ == "__main__":
    main()
