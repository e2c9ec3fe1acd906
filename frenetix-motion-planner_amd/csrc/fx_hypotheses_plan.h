// fx_hypotheses_plan.h -- how the obstacle stage of a finished step is run again over n_hyp prediction sets,
// as a pure function of its arguments: no HIP call, no environment, no allocation (tests/hypotheses_plan.cpp runs it without a GPU).
//
// One hypothesis = one set of obstacle tables (pack_obstacle_tables, fx_context.h) of the step's S, K:
//   hot [S][K][FX_HOT_STRIDE] | rec [S][K][12] | pmask [S] | hmask [S] | hot_gap_margin, 8-byte words, the set padded to 256 bytes.
// All tables of a call go up in ONE copy and stay in the block; what a ROUND of hypotheses adds is its scratch:
//   part [hyp][chunk][ld] f64   partial prediction sums of the item kernel
//   colm [hyp][chunk][tile] u64 collision ballots of the item kernel
//   tot  [hyp][ld] f64, colb [hyp][ld] u8   every candidate's total and collision decision (finish kernel -> selection kernel)
//   (cost, index) [hyp][n_part]  arg-min partials of the finish kernel's workgroups
// The rule: as many hypotheses per round as keep the round's tables plus its scratch within `limit` bytes (FX_ITEM_SCRATCH_BYTES,
// fx_pass.h), at least one, at most FX_HYP_GRID_Y (a launch's grid.y).  Three launches per round: items, finish, selection.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#define FX_HYP_MAX 4096          // hypotheses of one call
#define FX_HYP_GRID_Y 65535      // hypotheses of one round at most: they ride in grid.y
#define FX_HYP_FINISH_TILE 256   // candidates of a finish workgroup: one arg-min partial each
#define FX_HYP_HOT_STRIDE 10     // == FX_HOT_STRIDE (fx_device.h; fx_hypotheses_kernel.h asserts it)
#define FX_HYP_LAUNCHES_PER_ROUND 3

struct FxHypPlan {
    int32_t CH = 0, NC = 0;            // steps per item, chunks of the horizon
    int64_t n_tiles = 0;               // tiles of 64 candidates
    int64_t items = 0;                 // of one hypothesis: n_tiles x NC; grid.x of the item launch
    int64_t n_part = 0;                // finish workgroups per hypothesis; grid.x of the finish launch
    size_t table_words = 0;            // 8-byte words of one hypothesis' tables, padded to 256 bytes
    size_t scratch_bytes = 0;          // of one hypothesis in a round, every part padded to 256 bytes
    int32_t per_round = 0, rounds = 0;
    int32_t launches = 0;              // of the call
};

#if defined(__HIPCC__)
#define FX_HYP_HD __host__ __device__
#else
#define FX_HYP_HD
#endif

FX_HYP_HD inline size_t fx_hyp_pad(size_t bytes) { return (std::max<size_t>(bytes, 8) + 255) / 256 * 256; }

// offsets (8-byte words) of the parts of one hypothesis' tables
struct FxHypTable {
    size_t hot, rec, pm, hm, margin, words;
};
FX_HYP_HD inline FxHypTable fx_hyp_table(int S, int K) {   // (the item kernel calls it too)
    FxHypTable t;
    const size_t sk = (size_t)std::max(S, 0) * (size_t)std::max(K, 0);
    t.hot = 0;
    t.rec = t.hot + sk * FX_HYP_HOT_STRIDE;
    t.pm = t.rec + sk * 12;
    t.hm = t.pm + (size_t)std::max(S, 0);
    t.margin = t.hm + (size_t)std::max(S, 0);
    t.words = fx_hyp_pad((t.margin + 1) * 8) / 8;
    return t;
}

// C >= 0 candidates at leading dimension ld (C rounded up to 64, at least 64), S samples, 1 <= K <= 64 obstacles, CH steps per item,
// 1 <= n_hyp <= FX_HYP_MAX.  Returns false where one hypothesis' items exceed a launch's 2^31 - 1 workgroups.
inline bool fx_hypotheses_plan(int64_t C, int64_t ld, int S, int K, int CH, int32_t n_hyp, size_t limit, FxHypPlan &p) {
    p = FxHypPlan();
    C = std::max<int64_t>(C, 0);
    p.CH = std::max(CH, 1);
    const int steps = std::max(S - 1, 0);
    p.NC = std::max((steps + p.CH - 1) / p.CH, 1);
    p.n_tiles = std::max<int64_t>((C + 63) / 64, 1);
    p.items = p.n_tiles * p.NC;
    p.n_part = std::max<int64_t>((C + FX_HYP_FINISH_TILE - 1) / FX_HYP_FINISH_TILE, 1);
    p.table_words = fx_hyp_table(S, K).words;
    p.scratch_bytes = fx_hyp_pad(sizeof(double) * (size_t)p.NC * (size_t)ld) + fx_hyp_pad(8 * (size_t)p.NC * (size_t)p.n_tiles) +
                      fx_hyp_pad(sizeof(double) * (size_t)ld) + fx_hyp_pad((size_t)ld) + 2 * fx_hyp_pad(8 * (size_t)p.n_part);
    if (p.items > 0x7fffffffLL) return false;
    const size_t each = p.table_words * 8 + p.scratch_bytes;
    const size_t fit = std::max<size_t>(limit / each, 1);
    p.per_round = (int32_t)std::min<size_t>(std::min<size_t>(fit, FX_HYP_GRID_Y), (size_t)std::max<int32_t>(n_hyp, 1));
    p.rounds = (std::max<int32_t>(n_hyp, 1) + p.per_round - 1) / p.per_round;
    p.launches = FX_HYP_LAUNCHES_PER_ROUND * p.rounds;
    return true;
}

// what the launcher (fx_launch_hypotheses, fx_kernels.hip) gets of a ROUND: device pointers and sizes
struct FxHypArgs {
    // the step's (read only)
    const double *planes;       // [FX_NUM_PLANES][S][ld]
    const uint32_t *flags;      // [ld]
    const double *costmap;      // [n_cost][ld]
    int64_t C, ld;
    int32_t S, K;
    int32_t n_cost, n_pred;     // n_pred: position of FX_COST_PREDICTION in the cost list, -1 without one
    int32_t deferred;           // the sum's form: 1 with a prediction term (fx_cost_sum.h, the obstacle kernel's order)
    int32_t col_mode;           // the step ran the collision stage (FX_MODE_COLLISION with hulls)
    double w[16];               // the step's weights [n_cost] (FX_NUM_COSTS <= 16)
    double ox, oy;              // hot_origin
    double wb, half_len, half_wid;
    // the round's
    const double *tables;       // [n_hyp] tables of table_words words
    size_t table_words;
    int32_t n_hyp, CH, NC;
    int64_t n_tiles, n_part;
    double *part;               // [n_hyp][NC][ld]
    unsigned long long *colm;   // [n_hyp][NC][n_tiles]
    double *tot;                // [n_hyp][ld]
    unsigned char *colb;        // [n_hyp][ld]
    double *part_cost;          // [n_hyp][n_part]
    long long *part_idx;
    long long *winner;          // [n_hyp]
    double *cost;               // [n_hyp]
    long long *n_col;           // [n_hyp]
    double *out_pred, *out_total;   // [n_hyp][C] or null
    unsigned char *out_col;         // [n_hyp][C] or null
};
