// fx_rescore_plan.h -- how a re-score of n candidates under n_vec weight vectors is launched, as a pure
// function of its arguments: no HIP call, no environment, no allocation (tests/rescore_plan.cpp runs it without a GPU).
//
// Two regimes, chosen by the number of vectors alone:
//   FX_RESCORE_LANE    candidate per lane: workgroups of 256 candidates (tiles) x chunks of the vectors; a lane holds its candidate's
//                      raw costs in registers and loops over the chunk's vectors, the workgroup reduces (total, index) per vector.
//                      One partial per (vector, tile).
//   FX_RESCORE_VECTOR  vector per lane, from FX_RESCORE_VECTOR_MIN vectors -- a full wave of them -- on: one wave per (slice of the
//                      candidates, group of 64 vectors), every lane walks the slice with its own weights.  One partial per
//                      (vector, slice).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#define FX_RESCORE_LANE 1
#define FX_RESCORE_VECTOR 2
#define FX_RESCORE_TILE 256            // candidates of a lane-regime workgroup
#define FX_RESCORE_CHUNK_MAX 64        // vectors of a lane-regime workgroup at most (its LDS: one (cost, index) per vector and wave)
#define FX_RESCORE_VECTOR_MIN 64       // vectors from which a wave of them is full: the vector regime
#define FX_RESCORE_WORKGROUPS 512      // lane regime: the vectors are chunked finer while a call has fewer workgroups than this
#define FX_RESCORE_WAVES 2048          // vector regime: waves a call aims at (256 CUs x 4 SIMDs x 2)
#define FX_RESCORE_SLICE_MIN 32        // vector regime: candidates of a slice at least
#define FX_RESCORE_MAX_VECTORS 32768   // of one call (a launch's grid.y holds 65 535)

struct FxRescorePlan {
    int regime = 0;             // FX_RESCORE_LANE / FX_RESCORE_VECTOR
    int64_t n_part = 0;         // partials per vector: tiles (lane) or slices (vector); grid.x of the first launch
    int64_t per = 0;            // candidates per partial
    int32_t vec_chunk = 0;      // vectors per workgroup (lane: <= FX_RESCORE_CHUNK_MAX; vector: 64)
    int32_t grid_y = 0;         // chunks / groups of the vectors
    int32_t finish_blocks = 0;  // workgroups of the finish launch: four vectors each
};

// n >= 0 candidates (an agent without candidates still gets one, empty, partial per vector), 1 <= n_vec <= FX_RESCORE_MAX_VECTORS;
// forced: 0 the rule, FX_RESCORE_LANE / FX_RESCORE_VECTOR a test's or a measurement's choice.
inline FxRescorePlan fx_rescore_plan(int64_t n, int32_t n_vec, int forced) {
    FxRescorePlan p;
    n = std::max<int64_t>(n, 0);
    p.regime = (forced == FX_RESCORE_LANE || forced == FX_RESCORE_VECTOR) ? forced : (n_vec >= FX_RESCORE_VECTOR_MIN ? FX_RESCORE_VECTOR : FX_RESCORE_LANE);
    p.finish_blocks = (n_vec + 3) / 4;
    if (p.regime == FX_RESCORE_LANE) {
        p.per = FX_RESCORE_TILE;
        p.n_part = std::max<int64_t>((n + FX_RESCORE_TILE - 1) / FX_RESCORE_TILE, 1);
        int32_t vc = std::min<int32_t>(n_vec, FX_RESCORE_CHUNK_MAX);
        while (vc > 1 && p.n_part * ((n_vec + vc - 1) / vc) < FX_RESCORE_WORKGROUPS) vc = (vc + 1) / 2;
        p.vec_chunk = vc;
        p.grid_y = (n_vec + vc - 1) / vc;
    } else {
        p.vec_chunk = 64;
        p.grid_y = (n_vec + 63) / 64;
        const int64_t want = (FX_RESCORE_WAVES + p.grid_y - 1) / p.grid_y;
        const int64_t most = std::max<int64_t>((n + FX_RESCORE_SLICE_MIN - 1) / FX_RESCORE_SLICE_MIN, 1);
        const int64_t slices = std::min(want, most);
        p.per = std::max<int64_t>((n + slices - 1) / slices, 1);
        p.n_part = std::max<int64_t>((n + p.per - 1) / p.per, 1);   // (no slice without a candidate)
    }
    return p;
}

// what the launcher (fx_launch_rescore, fx_kernels.hip) gets of a call: device pointers and sizes
struct FxRescoreArgs {
    const double *costmap;     // [n_cost][ld] raw cost rows of the step
    const uint32_t *flags;     // [n]
    int64_t n, ld;
    int32_t n_cost, n_pred;    // n_pred: position of FX_COST_PREDICTION in the cost list, -1 without one
    int32_t deferred;          // the step closed its sum in the obstacle kernel (FX_MODE_INT_DEFER_OBST) and has a prediction term
    int32_t n_vec;
    const double *w;           // [n_vec][n_cost]
    double *part_cost;         // [n_vec][n_part]
    long long *part_idx;
    long long *winner;         // [n_vec]
    double *cost;              // [n_vec]
    double *totals;            // [n_vec][n], or null
};

// doubles + indices of the partials of such a call
inline size_t fx_rescore_partials(const FxRescorePlan &p, int32_t n_vec) { return (size_t)n_vec * (size_t)p.n_part; }
