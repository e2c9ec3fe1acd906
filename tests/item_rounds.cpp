// item_rounds.cpp -- the round rule of the passes that work in items over several agents (csrc/fx_pass.h, fx_item_rounds) and the
// table of such a call (fx_item_table) as a stand-alone host program (tests/test_item_rounds.py builds it with hipcc
// --cuda-host-only and holds its answers to the rules' statements).  Input, one case per line:
//   limit n_agents (n per_candidate_bytes items_per_tile)*
// Output per case, two lines:
//   case <segments> <fx_item_batch of the first agent, 0 without one> (agent round first count scratch_off)*
//   table <0, or fx_item_table's refusal> <scratch> <rounds> (row0 n_rows items fin_blocks)* <rows> (nb item0 fin0)* <agents> (agent_row)*
//   lookup <item indices checked> <of them wrong> <finish workgroups checked> <of them wrong> <first indices that do not ascend>
// (a refused table: "table <code>" alone, and "lookup -1"; a round of more than 2^24 items is not walked: "lookup -1" too).  Every
// row of an agent gets the agent's items per tile.  The lookup line applies the kernels' row search (row_of in
// fx_predprob_kernel.h, batch_row_of in fx_risk_kernel.h) to EVERY flat index of every round's item launch and finish launch.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fx_pass.h"

thread_local char g_err[512] = "";   // (the library's error text: fx_api.hip has it in the product)

// The kernels' rule as a plain loop: the last of a round's n_rows rows whose first index is at or before `at`.  The kernels count
// the rows with first0 <= at, 64 per ballot, and take the count minus one: the same row exactly when first0 ascends, so both are
// formed here and a difference counts as wrong.
template <typename T>
static int row_at(const T *first0, int n_rows, long long at) {
    int last = -1, count = 0;
    for (int k = 0; k < n_rows; k++)
        if ((long long)first0[k] <= at) { last = k; count++; }
    return last == count - 1 ? last : -2;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long limit;
        int n_agents;
        if (!(in >> limit >> n_agents)) continue;
        std::vector<FxItemAgent> agents((size_t)n_agents);
        std::vector<long long> per_tile((size_t)n_agents);
        for (size_t a = 0; a < agents.size(); a++) {
            long long n;
            unsigned long long per;
            in >> n >> per >> per_tile[a];
            agents[a] = FxItemAgent{(int64_t)n, (size_t)per};
        }
        const std::vector<FxItemSegment> segs = fx_item_rounds(agents.data(), n_agents, (size_t)limit);
        long long batch = 0;   // (fx_item_batch works on the library's own limit: comparable where the case uses it)
        if (n_agents > 0 && agents[0].per_candidate_bytes > 0) batch = (long long)fx_item_batch(agents[0].per_candidate_bytes, agents[0].n);
        printf("case %zu %lld", segs.size(), batch);
        for (const FxItemSegment &s : segs)
            printf(" %d %d %lld %lld %zu", (int)s.agent, (int)s.round, (long long)s.first, (long long)s.count, s.scratch_off);
        printf("\n");
        std::vector<int64_t> row_items(segs.size());
        for (size_t k = 0; k < segs.size(); k++) row_items[k] = (int64_t)per_tile[(size_t)segs[k].agent];
        FxItemTable t;
        const int rc = fx_item_table(segs, agents.data(), n_agents, row_items.data(), t);
        printf("table %d", rc);
        if (!rc) {
            printf(" %zu %zu", t.scratch, t.rounds.size());
            for (const FxItemRound &r : t.rounds) printf(" %d %d %lld %d", (int)r.row0, (int)r.n_rows, (long long)r.items, (int)r.fin_blocks);
            printf(" %zu", t.nb.size());
            for (size_t k = 0; k < t.nb.size(); k++) printf(" %lld %lld %d", (long long)t.nb[k], (long long)t.item0[k], (int)t.fin0[k]);
            printf(" %zu", t.agent_row.size());
            for (int32_t r : t.agent_row) printf(" %d", (int)r);
        }
        printf("\n");
        long long items = 0, items_bad = 0, fins = 0, fins_bad = 0, unsorted = 0;
        bool walk = !rc;
        for (const FxItemRound &r : t.rounds) walk = walk && r.items <= (1LL << 24);
        if (!walk) { printf("lookup -1\n"); continue; }
        for (const FxItemRound &r : t.rounds) {
            const int64_t *item0 = t.item0.data() + r.row0;
            const int32_t *fin0 = t.fin0.data() + r.row0;
            for (int k = 1; k < r.n_rows; k++) unsorted += (item0[k] < item0[k - 1]) + (fin0[k] < fin0[k - 1]);
            // the row whose [item0, item0 + items) holds the index, by walking the rows' own extents
            int row = 0;
            for (long long at = 0; at < r.items; at++, items++) {
                while (row + 1 < r.n_rows && at >= item0[row] + t.nb[(size_t)(r.row0 + row)] / 64 * row_items[(size_t)(r.row0 + row)]) row++;
                items_bad += row_at(item0, r.n_rows, at) != row;
            }
            row = 0;
            for (long long at = 0; at < r.fin_blocks; at++, fins++) {
                while (row + 1 < r.n_rows && at >= fin0[row] + (segs[(size_t)(r.row0 + row)].count + 255) / 256) row++;
                fins_bad += row_at(fin0, r.n_rows, at) != row;
            }
        }
        printf("lookup %lld %lld %lld %lld %lld\n", items, items_bad, fins, fins_bad, unsorted);
    }
    return 0;
}
