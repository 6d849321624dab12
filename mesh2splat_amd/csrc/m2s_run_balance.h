// m2s_run_balance.h — which dispatch slot every run of a launch in runs takes (RunInfo::order, m2s_device.h).
//
// Hardware workgroup h runs on XCD h % 8, so dispatch slot s belongs to the queue of XCD s % 8: XCD x works through the slots x, x + 8,
// x + 16, ... in that order.  A launch lasts until its slowest XCD has finished, so the eight queues should hold equal WORK (fragments),
// not only equal numbers of runs; and every queue should hold its heaviest runs first, so that what an XCD dispatches last — what the
// launch drains for — is light.
//
// The assignment: walk the runs from the heaviest to the lightest and give each to the queue that holds the fewest fragments so far and
// still has a free slot (longest processing time first, with a capacity per queue).  Runs reach a queue in rank order: every queue is
// non-increasing in weight.  n_slots is n_runs rounded up to whole groups of eight; the slots past the last run (slot i >= n_runs, which
// holds i: its workgroups exit at once) are the last slots of the queues n_runs % 8 ... 7, whose capacity is one run less.  Ties go to
// the queue with fewer runs, then to the higher XCD: equal loads deal a group of eight from XCD 7 down to XCD 0, which leans the
// heavier runs towards the queues that hold one run less.
//
// One function for the device (k_run_assign, m2s_kernels.hip: one lane) and the host (tests/test_run_balance.py compiles this header
// into a stand-alone program; tools/xcd_balance.py mirrors it): plain C++, no dynamic indexing of the eight queue registers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M2S_RB_HD __host__ __device__
#else
#define M2S_RB_HD
#endif

namespace m2s {
constexpr uint32_t kRunQueues = 8;   // XCDs of the device = queues of a launch in runs

// cost[r]: fragments of the run of rank r (r = 0: the heaviest; non-increasing), n_runs of them; n_slots: a multiple of 8 with
// n_runs <= n_slots < n_runs + 8.  order[slot] = rank of the run dispatched in that slot, for slot < n_runs; order[slot] = slot beyond.
M2S_RB_HD inline void run_balance_assign(const unsigned long long* cost, uint32_t n_runs, uint32_t n_slots, uint32_t* order) {
    unsigned long long load[kRunQueues];
    uint32_t used[kRunQueues], cap[kRunQueues];
    for (uint32_t x = 0; x < kRunQueues; ++x) {
        load[x] = 0ull;
        used[x] = 0u;
        cap[x] = n_runs > x ? (n_runs - x + kRunQueues - 1u) / kRunQueues : 0u;   // slots x, x + 8, ... below n_runs
    }
    for (uint32_t i = n_runs; i < n_slots; ++i) order[i] = i;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const unsigned long long c = cost[r];
        uint32_t best = kRunQueues, best_used = 0u;
        unsigned long long best_load = 0ull;
        for (uint32_t k = 0; k < kRunQueues; ++k) {
            const uint32_t x = kRunQueues - 1u - k;                  // from XCD 7 down: the first of equals wins
            const bool free_slot = used[x] < cap[x];
            const bool better = best == kRunQueues || load[x] < best_load || (load[x] == best_load && used[x] < best_used);
            if (free_slot && better) { best = x; best_load = load[x]; best_used = used[x]; }
        }
        // (the capacities add up to n_runs: a queue with a free slot exists)
        order[best_used * kRunQueues + best] = r;
        for (uint32_t x = 0; x < kRunQueues; ++x) {
            const bool hit = x == best;
            load[x] += hit ? c : 0ull;
            used[x] += hit ? 1u : 0u;
        }
    }
}
}  // namespace m2s
