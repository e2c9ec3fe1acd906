// fx_hypotheses_batch_plan.h -- how the hypotheses pass of SEVERAL agents in one call is launched, as a pure
// function of its arguments: no HIP call, no environment, no allocation but the tables it answers (tests/hypotheses_batch_plan.cpp
// runs it without a GPU).  The numbers of one agent stay in fx_hypotheses_plan.h; nothing of them is repeated here.
//
// An ENTRY is one listed agent with its own C, ld, S, K and n_hyp prediction sets.  A PAIR is (entry, hypothesis).  A ROW is one
// entry with a contiguous range of its hypotheses; per row the per-agent plan's numbers hold (NC, n_tiles, items, n_part,
// table_words, scratch_bytes), so its partials are laid out as in the per-agent call, inside the row's own segment of the round's
// scratch.  A ROUND takes pairs in call order while
//   * its tables plus its scratch -- table_words * 8 + scratch_bytes per pair -- stay within `limit` bytes, and
//   * none of its three flat grids exceeds FX_HYP_GRID_MAX workgroups: items (n_hyp x items per row), finish workgroups
//     (n_hyp x n_part per row), selection workgroups (one per pair);
// it holds at least one pair.  An entry's hypotheses may be cut across rounds: every pair's answer is independent of every other.
// Three launches per round whatever the number of entries.  A row's workgroups are consecutive in each grid; item0 / fin0 / sel0
// are its first ones, from 0 at the round's first row, ascending: what the kernels search (fxrisk::batch_row_of).
#pragma once

#include <vector>

#include "fx_hypotheses_plan.h"

#define FX_HYP_GRID_MAX 0x7fffffffLL   // workgroups of one launch

// refusals of fx_hypotheses_batch_plan (0: none); *bad receives the position of the entry in the call's list
#define FX_HYP_BATCH_NO_HYPOTHESIS 1   // n_hyp < 1
#define FX_HYP_BATCH_HYPOTHESES 2      // more than FX_HYP_MAX hypotheses for one agent
#define FX_HYP_BATCH_GRID 3            // one hypothesis' items above FX_HYP_GRID_MAX

// what the call gives of an entry
struct FxHypBatchItem {
    int64_t C, ld;
    int32_t S, K, n_hyp;
};

// the parts of a row's segment of the round's scratch, bytes from the segment's start: the per-agent call's arrays with the row's
// R hypotheses in front -- part [R][NC][ld] | colm [R][NC][n_tiles] | tot [R][ld] | colb [R][ld] | (cost, index) [R][n_part]
struct FxHypSegment {
    size_t part, colm, tot, colb, part_cost, part_idx, bytes;
};
inline FxHypSegment fx_hyp_batch_segment(const FxHypPlan &p, int64_t ld, int32_t R) {
    FxHypSegment g;
    const size_t r = (size_t)R, l = (size_t)ld;
    g.part = 0;
    g.colm = g.part + fx_hyp_pad(sizeof(double) * r * (size_t)p.NC * l);
    g.tot = g.colm + fx_hyp_pad(8 * r * (size_t)p.NC * (size_t)p.n_tiles);
    g.colb = g.tot + fx_hyp_pad(sizeof(double) * r * l);
    g.part_cost = g.colb + fx_hyp_pad(r * l);
    g.part_idx = g.part_cost + fx_hyp_pad(8 * r * (size_t)p.n_part);
    g.bytes = g.part_idx + fx_hyp_pad(8 * r * (size_t)p.n_part);   // <= R x p.scratch_bytes: that pads every part per hypothesis
    return g;
}

struct FxHypBatchRow {
    int32_t entry, round;     // position in the call's list; rounds count from 0
    int32_t h0, n_hyp;        // hypotheses [h0, h0 + n_hyp) of the entry
    int64_t item0, fin0, sel0;   // first workgroup in each of its round's three launches
    size_t table_off;         // bytes: its first table among the call's tables, which stand in call order
    size_t scratch_off;       // bytes: its segment in the round's scratch, n_hyp x the entry's scratch_bytes long
    int64_t out0;             // its first answer among the call's concatenated answers
};

struct FxHypBatchRound {
    int32_t row0 = 0, n_rows = 0;   // rows [row0, row0 + n_rows), consecutive and in call order
    int32_t K_max = 0;              // largest K among its rows: sizes the item launch's LDS
    int64_t items = 0, fin_blocks = 0, pairs = 0;   // the three grids
    size_t bytes = 0, scratch = 0;  // tables plus scratch; scratch alone
};

struct FxHypBatchPlan {
    std::vector<FxHypPlan> plans;   // [entries]: fx_hypotheses_plan of the entry alone (per_round, rounds, launches: of a per-agent call)
    std::vector<int64_t> out0;      // [entries]: the entry's first answer
    std::vector<size_t> table0;     // [entries]: bytes, the entry's first table
    std::vector<FxHypBatchRow> rows;
    std::vector<FxHypBatchRound> rounds;
    int32_t CH = 0;
    int64_t pairs = 0;              // of the call
    size_t table_bytes = 0;         // all tables of the call
    size_t scratch = 0;             // of the largest round
    int32_t launches = 0;           // FX_HYP_LAUNCHES_PER_ROUND x rounds
};

inline int fx_hypotheses_batch_plan(const FxHypBatchItem *items, int n_items, int CH, size_t limit, FxHypBatchPlan &t, int *bad) {
    t = FxHypBatchPlan{};
    const size_t E = (size_t)std::max(n_items, 0);
    t.plans.resize(E), t.out0.resize(E), t.table0.resize(E);
    for (size_t i = 0; i < E; i++) {
        if (bad) *bad = (int)i;
        const FxHypBatchItem &it = items[i];
        if (it.n_hyp < 1) return FX_HYP_BATCH_NO_HYPOTHESIS;
        if (it.n_hyp > FX_HYP_MAX) return FX_HYP_BATCH_HYPOTHESES;
        if (!fx_hypotheses_plan(it.C, it.ld, it.S, it.K, CH, it.n_hyp, limit, t.plans[i])) return FX_HYP_BATCH_GRID;
        t.CH = t.plans[i].CH;
    }
    FxHypBatchRound rd;
    for (size_t i = 0; i < E; i++) {
        const FxHypBatchItem &it = items[i];
        const FxHypPlan &p = t.plans[i];
        const size_t each = p.table_words * 8 + p.scratch_bytes;
        t.out0[i] = t.pairs, t.table0[i] = t.table_bytes;
        for (int32_t h = 0; h < it.n_hyp; h++) {
            // (one pair's grids are within the limit: items was checked, n_part <= items, and a pair selects in one workgroup)
            const bool full = rd.pairs > 0 && (each > limit - std::min(rd.bytes, limit) || rd.items + p.items > FX_HYP_GRID_MAX ||
                                               rd.fin_blocks + p.n_part > FX_HYP_GRID_MAX || rd.pairs + 1 > FX_HYP_GRID_MAX);
            if (full) {
                t.rounds.push_back(rd);
                rd = FxHypBatchRound{};
                rd.row0 = (int32_t)t.rows.size();
            }
            if (rd.n_rows == 0 || t.rows.back().entry != (int32_t)i) {
                t.rows.push_back(FxHypBatchRow{(int32_t)i, (int32_t)t.rounds.size(), h, 0, rd.items, rd.fin_blocks, rd.pairs, t.table_bytes,
                                               rd.scratch, t.pairs});
                rd.n_rows++;
                rd.K_max = std::max(rd.K_max, it.K);
            }
            t.rows.back().n_hyp++;
            rd.items += p.items, rd.fin_blocks += p.n_part, rd.pairs++;
            rd.bytes += each, rd.scratch += p.scratch_bytes;
            t.pairs++, t.table_bytes += p.table_words * 8;
            t.scratch = std::max(t.scratch, rd.scratch);
        }
    }
    if (rd.pairs > 0) t.rounds.push_back(rd);
    t.launches = FX_HYP_LAUNCHES_PER_ROUND * (int32_t)t.rounds.size();
    return 0;
}

// (row, hypothesis of the row, tile, chunk) of workgroup `at` of a round's item launch: the kernel's search (the last row that
// starts at or before `at`) and its divisions, on the host -- what tests/hypotheses_batch_plan.cpp holds the table to
inline void fx_hyp_batch_locate(const FxHypBatchPlan &t, int round, int64_t at, int *row, int *h, int64_t *tile, int *chunk) {
    const FxHypBatchRound &rd = t.rounds[round];
    int r = rd.row0;
    for (int k = rd.row0; k < rd.row0 + rd.n_rows; k++)
        if (t.rows[k].item0 <= at) r = k;
    const FxHypPlan &p = t.plans[t.rows[r].entry];
    const int64_t local = at - t.rows[r].item0, rest = local % p.items;
    *row = r, *h = (int)(local / p.items), *tile = rest / p.NC, *chunk = (int)(rest % p.NC);
}

// One row as the kernels read it (device memory; fx_hypotheses_batch_kernel.h): the per-agent launch's arguments with the row's
// own pointers -- tables at its first hypothesis, the arrays of its scratch segment, its answers and its blocks of the rows asked
// for -- and its first workgroups
struct FxHypBatchDevRow {
    FxHypArgs a;
    int64_t item0, fin0, sel0;
    int64_t items;   // of one hypothesis: a.n_tiles x a.NC
};

// what the launcher (fx_launch_hypotheses_batch, fx_kernels.hip) gets of a ROUND
struct FxHypBatchArgs {
    const FxHypBatchDevRow *rows;             // [n_rows] of the round
    const int64_t *item0, *fin0, *sel0;       // [n_rows] each, ascending from 0
    int32_t n_rows, CH;
    int64_t items, fin_blocks, pairs;         // the three grids
    size_t lds_bytes;                         // CH x K_max x 48
};
