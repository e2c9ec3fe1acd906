// item_rounds.cpp -- the round rule of the passes that work in items over several agents (csrc/fx_pass.h, fx_item_rounds) as a
// stand-alone host program (tests/test_item_rounds.py builds it with hipcc --cuda-host-only and holds its answers to the rule's
// statement).  Input, one case per line: limit n_agents (n per_candidate_bytes)*.  Output per case: one line
//   case <segments> <fx_item_batch of the first agent, 0 without one> (agent round first count scratch_off)*
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fx_pass.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long limit;
        int n_agents;
        if (!(in >> limit >> n_agents)) continue;
        std::vector<FxItemAgent> agents((size_t)n_agents);
        for (auto &a : agents) {
            long long n;
            unsigned long long per;
            in >> n >> per;
            a = FxItemAgent{(int64_t)n, (size_t)per};
        }
        const std::vector<FxItemSegment> segs = fx_item_rounds(agents.data(), n_agents, (size_t)limit);
        long long batch = 0;   // (fx_item_batch works on the library's own limit: comparable where the case uses it)
        if (n_agents > 0 && agents[0].per_candidate_bytes > 0) batch = (long long)fx_item_batch(agents[0].per_candidate_bytes, agents[0].n);
        printf("case %zu %lld", segs.size(), batch);
        for (const FxItemSegment &s : segs)
            printf(" %d %d %lld %lld %zu", (int)s.agent, (int)s.round, (long long)s.first, (long long)s.count, s.scratch_off);
        printf("\n");
    }
    return 0;
}
