// rescore_batch_plan.cpp -- the launch table of the batched re-score (csrc/fx_rescore_batch_plan.h, fx_rescore_batch_plan and
// fx_rescore_batch_locate) as a stand-alone host program (tests/test_rescore_batch_plan.py builds it with hipcc --cuda-host-only and
// holds its answers to the table's statement).  Input, one call per line:
//   forced n_entries  n_0 n_vec_0  n_1 n_vec_1 ...
// Output per call:
//   batch <rc> <bad> <n_lane> <n_vector> <lane_wgs> <vector_wgs> <partials> <vectors> <finish_blocks>
// and, where rc is 0, per entry in call order
//   row <regime> <n_part> <per> <vec_chunk> <grid_y> <slot> <wg0> <part0> <fin0> <out0> <partials of the entry's own plan>
// and per workgroup of each regime's launch -- every one up to FX_LOCATE_ALL workgroups of a launch, beyond that the first and the
// last of every entry --
//   wg <regime> <workgroup> <entry> <tile or slice> <chunk or group>
// First of all one line: constants <rows> <grid_max> <max_vectors>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fx_rescore_batch_plan.h"

#define FX_LOCATE_ALL 100000

static void locate(const FxRescoreBatchPlan &t, int regime, int64_t wg) {
    int entry;
    int64_t part, chunk;
    fx_rescore_batch_locate(t, regime, wg, &entry, &part, &chunk);
    printf("wg %d %lld %d %lld %lld\n", regime, (long long)wg, entry, (long long)part, (long long)chunk);
}

int main() {
    printf("constants %d %lld %d\n", (int)FX_RESCORE_ROWS, (long long)FX_RESCORE_GRID_MAX, FX_RESCORE_MAX_VECTORS);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int forced, n_entries;
        if (!(in >> forced >> n_entries)) continue;
        std::vector<FxRescoreBatchItem> items((size_t)n_entries);
        for (FxRescoreBatchItem &it : items) {
            long long n;
            int w;
            in >> n >> w;
            it = FxRescoreBatchItem{(int64_t)n, (int32_t)w};
        }
        FxRescoreBatchPlan t;
        int bad = -1;
        const int rc = fx_rescore_batch_plan(items.data(), n_entries, forced, t, &bad);
        printf("batch %d %d %d %d %lld %lld %lld %lld %lld\n", rc, bad, (int)t.n_lane, (int)t.n_vector, (long long)t.lane_wgs, (long long)t.vector_wgs,
               (long long)t.partials, (long long)t.vectors, (long long)t.finish_blocks);
        if (rc) continue;
        for (int i = 0; i < n_entries; i++) {
            const FxRescoreBatchRow &r = t.rows[i];
            printf("row %d %lld %lld %d %d %d %lld %lld %lld %lld %zu\n", r.plan.regime, (long long)r.plan.n_part, (long long)r.plan.per,
                   (int)r.plan.vec_chunk, (int)r.plan.grid_y, (int)r.slot, (long long)r.wg0, (long long)r.part0, (long long)r.fin0, (long long)r.out0,
                   fx_rescore_partials(r.plan, items[i].n_vec));
        }
        for (int regime : {FX_RESCORE_LANE, FX_RESCORE_VECTOR}) {
            const int64_t wgs = regime == FX_RESCORE_LANE ? t.lane_wgs : t.vector_wgs;
            if (wgs <= FX_LOCATE_ALL) {
                for (int64_t wg = 0; wg < wgs; wg++) locate(t, regime, wg);
            } else {
                for (int i = 0; i < n_entries; i++) {
                    const FxRescoreBatchRow &r = t.rows[i];
                    if (r.plan.regime != regime) continue;
                    locate(t, regime, r.wg0);
                    locate(t, regime, r.wg0 + r.plan.n_part * r.plan.grid_y - 1);
                }
            }
        }
    }
    return 0;
}
