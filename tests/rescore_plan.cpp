// rescore_plan.cpp -- the launch rule of the re-score pass (csrc/fx_rescore_plan.h, fx_rescore_plan) as a stand-alone host program
// (tests/test_rescore_plan.py builds it with hipcc --cuda-host-only and holds its answers to the rule's statement).  Input, one case
// per line:
//   n n_vec forced
// Output per case:
//   plan <regime> <n_part> <per> <vec_chunk> <grid_y> <finish_blocks> <partials>
// and first of all one line with the constants the rule is made of:
//   constants <lane> <vector> <tile> <chunk_max> <vector_min> <workgroups> <waves> <slice_min> <max_vectors>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fx_rescore_plan.h"

int main() {
    printf("constants %d %d %d %d %d %d %d %d %d\n", FX_RESCORE_LANE, FX_RESCORE_VECTOR, FX_RESCORE_TILE, FX_RESCORE_CHUNK_MAX, FX_RESCORE_VECTOR_MIN,
           FX_RESCORE_WORKGROUPS, FX_RESCORE_WAVES, FX_RESCORE_SLICE_MIN, FX_RESCORE_MAX_VECTORS);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long n;
        int n_vec, forced;
        if (!(in >> n >> n_vec >> forced)) continue;
        const FxRescorePlan p = fx_rescore_plan((int64_t)n, (int32_t)n_vec, forced);
        printf("plan %d %lld %lld %d %d %d %zu\n", p.regime, (long long)p.n_part, (long long)p.per, (int)p.vec_chunk, (int)p.grid_y, (int)p.finish_blocks,
               fx_rescore_partials(p, n_vec));
    }
    return 0;
}
