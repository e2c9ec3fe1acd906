// hypotheses_batch_plan.cpp -- the rows and rounds of the hypotheses pass over several agents (csrc/fx_hypotheses_batch_plan.h,
// fx_hypotheses_batch_plan) as a stand-alone host program (tests/test_hypotheses_batch_plan.py builds it with the host compiler and
// holds its answers to the rule's statement).
// Input, one call per line:
//   limit CH n_entries  then per entry  C S K n_hyp
// Output per call:
//   call <rc> <bad> <CH> <entries> <rows> <rounds> <pairs> <table_bytes> <scratch> <launches>
// and, where rc == 0,
//   entry <i> <NC> <n_tiles> <items> <n_part> <table_words> <scratch_bytes> <out0> <table0> | the same six of fx_hypotheses_plan alone
//   row <entry> <round> <h0> <n_hyp> <item0> <fin0> <sel0> <table_off> <scratch_off> <out0> <segment bytes>
//   round <row0> <n_rows> <K_max> <items> <fin_blocks> <pairs> <bytes> <scratch>
//   locate <round> <at> <row> <h> <tile> <chunk>      for the first and last item of every row of at most 64 rows
// and first of all one line with the constants:
//   constants <max hypotheses> <grid max> <launches per round>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fx_hypotheses_batch_plan.h"

int main() {
    printf("constants %d %lld %d\n", FX_HYP_MAX, (long long)FX_HYP_GRID_MAX, FX_HYP_LAUNCHES_PER_ROUND);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned long long limit;
        int CH, n;
        if (!(in >> limit >> CH >> n)) continue;
        std::vector<FxHypBatchItem> items((size_t)n);
        for (int i = 0; i < n; i++) {
            long long C;
            int S, K, H;
            in >> C >> S >> K >> H;
            items[i] = FxHypBatchItem{(int64_t)C, (int64_t)(((C > 1 ? C : 1) + 63) / 64 * 64), S, K, H};
        }
        FxHypBatchPlan t;
        int bad = -1;
        const int rc = fx_hypotheses_batch_plan(items.data(), n, CH, (size_t)limit, t, &bad);
        printf("call %d %d %d %d %zu %zu %lld %zu %zu %d\n", rc, bad, (int)t.CH, n, rc ? 0 : t.rows.size(), rc ? 0 : t.rounds.size(),
               (long long)t.pairs, t.table_bytes, t.scratch, (int)t.launches);
        if (rc) continue;
        for (int i = 0; i < n; i++) {
            const FxHypPlan &p = t.plans[i];
            FxHypPlan q;
            fx_hypotheses_plan(items[i].C, items[i].ld, items[i].S, items[i].K, CH, items[i].n_hyp, (size_t)limit, q);
            printf("entry %d %d %lld %lld %lld %zu %zu %lld %zu | %d %lld %lld %lld %zu %zu\n", i, (int)p.NC, (long long)p.n_tiles,
                   (long long)p.items, (long long)p.n_part, p.table_words, p.scratch_bytes, (long long)t.out0[i], t.table0[i], (int)q.NC,
                   (long long)q.n_tiles, (long long)q.items, (long long)q.n_part, q.table_words, q.scratch_bytes);
        }
        for (const FxHypBatchRow &r : t.rows)
            printf("row %d %d %d %d %lld %lld %lld %zu %zu %lld %zu\n", (int)r.entry, (int)r.round, (int)r.h0, (int)r.n_hyp, (long long)r.item0,
                   (long long)r.fin0, (long long)r.sel0, r.table_off, r.scratch_off, (long long)r.out0,
                   fx_hyp_batch_segment(t.plans[r.entry], items[r.entry].ld, r.n_hyp).bytes);
        for (const FxHypBatchRound &rd : t.rounds)
            printf("round %d %d %d %lld %lld %lld %zu %zu\n", (int)rd.row0, (int)rd.n_rows, (int)rd.K_max, (long long)rd.items,
                   (long long)rd.fin_blocks, (long long)rd.pairs, rd.bytes, rd.scratch);
        if (t.rows.size() <= 64)
            for (size_t k = 0; k < t.rows.size(); k++) {
                const FxHypBatchRow &r = t.rows[k];
                const int64_t last = r.item0 + (int64_t)r.n_hyp * t.plans[r.entry].items - 1;
                for (int64_t at : {r.item0, last}) {
                    int row, h, chunk;
                    int64_t tile;
                    fx_hyp_batch_locate(t, r.round, at, &row, &h, &tile, &chunk);
                    printf("locate %d %lld %d %d %lld %d\n", (int)r.round, (long long)at, row, h, (long long)tile, chunk);
                }
            }
    }
    return 0;
}
