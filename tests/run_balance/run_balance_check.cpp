// TEST INFRASTRUCTURE (tests/test_run_balance.py): the shipped run_balance_assign (mesh2splat_amd/csrc/m2s_run_balance.h) as a host
// program.  Standard input: any number of cases "n_runs n_slots cost[0] ... cost[n_runs - 1]" (costs in rank order); standard output:
// one line per case, order[0] ... order[n_slots - 1].  Every array has exactly the size the function is promised, so that a build with
// -fsanitize=address,undefined sees any access past it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "m2s_run_balance.h"

int main() {
    unsigned n_runs = 0, n_slots = 0;
    while (std::scanf("%u %u", &n_runs, &n_slots) == 2) {
        if (n_slots % 8u != 0u || n_runs > n_slots || n_slots - n_runs >= 8u) { std::fprintf(stderr, "bad case %u %u\n", n_runs, n_slots); return 2; }
        std::vector<unsigned long long> cost(n_runs);
        for (unsigned i = 0; i < n_runs; ++i)
            if (std::scanf("%llu", &cost[i]) != 1) { std::fprintf(stderr, "short case\n"); return 2; }
        std::vector<uint32_t> order(n_slots, 0xFFFFFFFFu);
        m2s::run_balance_assign(cost.data(), n_runs, n_slots, order.data());
        for (unsigned i = 0; i < n_slots; ++i) std::printf(i + 1 < n_slots ? "%u " : "%u", order[i]);
        std::printf("\n");
    }
    return 0;
}
