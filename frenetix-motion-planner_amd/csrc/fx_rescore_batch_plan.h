// fx_rescore_batch_plan.h -- how a re-score of SEVERAL agents in one call is launched, as a pure function of
// its arguments: no HIP call, no environment, no allocation but the table it answers (tests/rescore_batch_plan.cpp runs it without a
// GPU).  The launch rule of one agent stays in fx_rescore_plan.h; nothing of it is repeated here.
//
// An ENTRY is one listed agent with its own n candidates and n_vec weight vectors.  Every entry takes the regime and the launch shape
// fx_rescore_plan gives it alone, so its partials are laid out as in the per-agent call.  The entries of a regime share ONE launch
// with a flat 1-D grid: an entry's workgroups are consecutive, workgroup `local` of an entry is (tile or slice = local % n_part,
// chunk or group = local / n_part) -- what (blockIdx.x, blockIdx.y) are in the per-agent launch.  The finish launch has a wave per
// (entry, vector), four waves a workgroup, flat over all entries.
#pragma once

#include <vector>

#include "../../include/fxplan.h"
#include "fx_rescore_plan.h"

#define FX_RESCORE_ROWS (FX_NUM_COSTS + 1)   // entries of an effective cost list at most: the step's own list and the responsibility term
#define FX_RESCORE_GRID_MAX 0x7fffffffLL     // workgroups of one launch

// refusals of fx_rescore_batch_plan (0: none); *bad receives the position of the entry in the call's list
#define FX_RESCORE_BATCH_NO_VECTOR 1     // n_vec < 1
#define FX_RESCORE_BATCH_VECTORS 2       // more than FX_RESCORE_MAX_VECTORS vectors for one agent
#define FX_RESCORE_BATCH_GRID 3          // a flat grid above FX_RESCORE_GRID_MAX

// what the call gives of an entry
struct FxRescoreBatchItem {
    int64_t n;        // candidates
    int32_t n_vec;    // weight vectors
};

// what the rule answers for it
struct FxRescoreBatchRow {
    FxRescorePlan plan;   // of the entry alone
    int32_t slot;         // position in the device table: the lane-regime entries first, then the vector-regime ones, each in call order
    int64_t wg0;          // first workgroup in its regime's launch
    int64_t part0;        // first of its n_vec x plan.n_part partials in the call's partial buffers
    int64_t fin0;         // first wave of the finish launch: waves follow the device table
    int64_t out0;         // first of its n_vec winners / costs in the call's concatenated outputs: call order
};

struct FxRescoreBatchPlan {
    std::vector<FxRescoreBatchRow> rows;   // [entries], call order
    std::vector<int32_t> order;            // [entries]: order[slot] = position in the call's list
    int32_t n_lane = 0, n_vector = 0;      // entries of each regime: device slots [0, n_lane) and [n_lane, n_lane + n_vector)
    int64_t lane_wgs = 0, vector_wgs = 0;  // grid of each regime's launch (0: no launch)
    int64_t partials = 0, vectors = 0;     // of the whole call
    int64_t finish_blocks = 0;             // ceil(vectors / 4)
};

// forced: 0 the rule per entry, FX_RESCORE_LANE / FX_RESCORE_VECTOR every entry in that regime (a test's or a measurement's choice)
inline int fx_rescore_batch_plan(const FxRescoreBatchItem *items, int n_items, int forced, FxRescoreBatchPlan &t, int *bad) {
    t = FxRescoreBatchPlan{};
    t.rows.resize((size_t)std::max(n_items, 0));
    t.order.resize(t.rows.size());
    for (int i = 0; i < n_items; i++) {
        if (bad) *bad = i;
        if (items[i].n_vec < 1) return FX_RESCORE_BATCH_NO_VECTOR;
        if (items[i].n_vec > FX_RESCORE_MAX_VECTORS) return FX_RESCORE_BATCH_VECTORS;
        FxRescoreBatchRow &r = t.rows[i];
        r.plan = fx_rescore_plan(items[i].n, items[i].n_vec, forced);
        if (r.plan.n_part > FX_RESCORE_GRID_MAX) return FX_RESCORE_BATCH_GRID;
        (r.plan.regime == FX_RESCORE_LANE ? t.n_lane : t.n_vector)++;
        r.out0 = t.vectors;
        t.vectors += items[i].n_vec;
    }
    int32_t lane = 0, vec = t.n_lane;
    for (int i = 0; i < n_items; i++) {
        FxRescoreBatchRow &r = t.rows[i];
        r.slot = r.plan.regime == FX_RESCORE_LANE ? lane++ : vec++;
        t.order[r.slot] = i;
    }
    for (int s = 0; s < n_items; s++) {   // (device order: the offsets a kernel searches ascend with the slot)
        FxRescoreBatchRow &r = t.rows[t.order[s]];
        const FxRescoreBatchItem &it = items[t.order[s]];
        if (bad) *bad = t.order[s];
        int64_t &wgs = r.plan.regime == FX_RESCORE_LANE ? t.lane_wgs : t.vector_wgs;
        r.wg0 = wgs;
        wgs += r.plan.n_part * r.plan.grid_y;   // (n_part < 2^31, grid_y < 2^16, entries < 2^31: no overflow before the check)
        if (wgs > FX_RESCORE_GRID_MAX) return FX_RESCORE_BATCH_GRID;
        r.part0 = t.partials;
        t.partials += (int64_t)fx_rescore_partials(r.plan, it.n_vec);
        r.fin0 = s == 0 ? 0 : t.rows[t.order[s - 1]].fin0 + items[t.order[s - 1]].n_vec;
    }
    t.finish_blocks = (t.vectors + 3) / 4;
    if (t.finish_blocks > FX_RESCORE_GRID_MAX) return FX_RESCORE_BATCH_GRID;
    return 0;
}

// (entry, tile or slice, chunk or group) of workgroup wg of a regime's launch: the kernels' search (the last entry of the regime that
// starts at or before wg) and their divisions, on the host -- what tests/rescore_batch_plan.cpp holds the table to
inline void fx_rescore_batch_locate(const FxRescoreBatchPlan &t, int regime, int64_t wg, int *entry, int64_t *part, int64_t *chunk) {
    const int s0 = regime == FX_RESCORE_LANE ? 0 : t.n_lane, s1 = regime == FX_RESCORE_LANE ? t.n_lane : t.n_lane + t.n_vector;
    int s = s0;
    for (int k = s0; k < s1; k++)
        if (t.rows[t.order[k]].wg0 <= wg) s = k;
    const FxRescoreBatchRow &r = t.rows[t.order[s]];
    const int64_t local = wg - r.wg0;
    *entry = t.order[s], *part = local % r.plan.n_part, *chunk = local / r.plan.n_part;
}

// Position of the responsibility term in a cost list of n_cost ascending ids: in front of the first entry whose id is above
// FX_COST_PREDICTION -- its place in the name-sorted list, between `prediction` and `velocity_offset` -- else at the end.  The one
// statement of that rule: the responsibility pass (fx_api_risk.hip) and the re-score with external rows.
inline int fx_resp_term_at(const int32_t *cost_id, int n_cost) {
    int at = n_cost;
    for (int m = n_cost - 1; m >= 0; m--)
        if (cost_id[m] > FX_COST_PREDICTION) at = m;
    return at;
}

// One entry as the kernels read it (device memory; fx_rescore_batch_kernel.h).  row[m]: base of the candidates' values of entry m of
// the effective list -- costmap + m' * ld of the step's own row, or an external row's device address; the kernels need not know which.
struct FxRescoreEntry {
    const double *row[FX_RESCORE_ROWS];
    const uint32_t *flags;      // [n]
    const double *w;            // [n_vec][n_cost]
    double *part_cost;          // [n_vec][n_part]
    long long *part_idx;
    long long *winner;          // [n_vec]
    double *cost;               // [n_vec]
    double *totals;             // [n_vec][n], or null
    int64_t n, n_part, per;     // candidates; partials per vector; candidates per slice (vector regime)
    int64_t wg0, fin0;          // first workgroup in its launch, first wave in the finish launch
    int32_t n_cost, n_pred;     // entries of the EFFECTIVE list; position of the prediction in it, -1 without one
    int32_t deferred;           // as FxRescoreArgs.deferred
    int32_t n_vec, vec_chunk;   // vectors; of a lane-regime workgroup
    int32_t pad_;
};

// what the launcher (fx_launch_rescore_batch, fx_kernels.hip) gets of a call
struct FxRescoreBatchArgs {
    const FxRescoreEntry *entries;   // device table, lane-regime entries first
    const int64_t *wg0;              // [n_lane + n_vector] the entries' first workgroups (each regime from 0), [.. + n_lane + n_vector] their first waves
    int32_t n_lane, n_vector;
    int64_t lane_wgs, vector_wgs, finish_blocks, n_waves;   // grids of the three launches; waves of the finish launch: all vectors
    // the totals of vector-regime entries come from the lane kernel without its reduction, as in fx_launch_rescore: their own table
    const FxRescoreEntry *tot_entries;
    const int64_t *tot_wg0;
    int32_t n_tot;
    int64_t tot_wgs;
};
