// hypotheses_plan.cpp -- the launch rule of the hypotheses pass (csrc/fx_hypotheses_plan.h, fx_hypotheses_plan) as a stand-alone host
// program (tests/test_hypotheses_plan.py builds it with hipcc --cuda-host-only and holds its answers to the rule's statement).
// Input, one case per line:
//   C S K CH n_hyp limit
// Output per case:
//   plan <ok> <CH> <NC> <n_tiles> <items> <n_part> <table_words> <scratch_bytes> <per_round> <rounds> <launches>
//   table <hot> <rec> <pm> <hm> <margin> <words>
// and first of all one line with the constants the rule is made of:
//   constants <max> <grid_y> <finish_tile> <hot_stride> <launches_per_round>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fx_hypotheses_plan.h"

int main() {
    printf("constants %d %d %d %d %d\n", FX_HYP_MAX, FX_HYP_GRID_Y, FX_HYP_FINISH_TILE, FX_HYP_HOT_STRIDE, FX_HYP_LAUNCHES_PER_ROUND);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long C, limit;
        int S, K, CH, n_hyp;
        if (!(in >> C >> S >> K >> CH >> n_hyp >> limit)) continue;
        const long long ld = ((C > 1 ? C : 1) + 63) / 64 * 64;
        FxHypPlan p;
        const bool ok = fx_hypotheses_plan((int64_t)C, (int64_t)ld, S, K, CH, (int32_t)n_hyp, (size_t)limit, p);
        printf("plan %d %d %d %lld %lld %lld %zu %zu %d %d %d\n", (int)ok, (int)p.CH, (int)p.NC, (long long)p.n_tiles, (long long)p.items,
               (long long)p.n_part, p.table_words, p.scratch_bytes, (int)p.per_round, (int)p.rounds, (int)p.launches);
        const FxHypTable t = fx_hyp_table(S, K);
        printf("table %zu %zu %zu %zu %zu %zu\n", t.hot, t.rec, t.pm, t.hm, t.margin, t.words);
    }
    return 0;
}
