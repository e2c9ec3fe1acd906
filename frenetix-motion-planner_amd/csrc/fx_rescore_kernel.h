// fx_rescore_kernel.h -- a finished plan step re-scored under many cost-weight vectors at once, beside the step: nothing a step wrote
// is rewritten (host: fx_api_rescore.hip; launch rule: fx_rescore_plan.h).
//
// total(c) under a vector w is what the step would have stored as cost[c] had it run with w: FxCostSum (fx_cost_sum.h) over the
// candidate's raw cost rows [n_cost][ld], NaN without FX_FLAG_COSTED.  winner(w) is the lexicographic (total, index) minimum over
// the candidates with FX_FLAG_SELECTABLE and neither FX_FLAG_COLLISION nor FX_FLAG_BOUNDARY, NaN totals skipped (fx_select.h);
// indices are the agent's local ones.  FP64, no atomics: the same bits on every run and in both regimes.
//
//   fx_rescore_lane_kernel    candidate per lane.  One coalesced load per row per wave; the lane's n_cost raw costs and its flag word
//                             stay in registers while it loops over the chunk's vectors, whose weights are wave-uniform.  Per
//                             vector the waves reduce (total, index), thread v of the workgroup combines the four waves of vector v
//                             in wave order: partial[v][tile].  Writes totals[v][c] where asked, coalesced; REDUCE = false is the
//                             totals alone (what the vector regime launches beside its own kernel when a caller wants them: a
//                             lane per vector would store them at a stride of n doubles).
//   fx_rescore_vector_kernel  vector per lane.  A wave owns 64 vectors and a slice of the candidates; flag word and rows of a
//                             candidate are wave-uniform loads, every lane keeps its own running (best, index) with a strict <
//                             while the indices ascend -- ties go to the lower index, no cross-lane reduction: partial[v][slice].
//   fx_rescore_finish_kernel  one wave per vector reduces its partials: winner[v] (-1: nothing eligible), cost[v] (+inf then).
#pragma once

#include <hip/hip_runtime.h>

#include "fx_cost_sum.h"
#include "fx_rescore_plan.h"
#include "fx_select.h"

namespace fxrs {

// what the kernels read of a call beside its pointers
struct Dims {
    int64_t n, ld;             // candidates, leading dimension of the cost rows
    int32_t n_cost, n_pred;    // n_pred: position of FX_COST_PREDICTION in the cost list, -1 without one
    int32_t deferred;          // the step closed its sum in the obstacle kernel (FX_MODE_INT_DEFER_OBST) and has a prediction term
    int32_t n_vec, vec_chunk;  // vectors of the call, of a lane-regime workgroup
    int64_t n_part, per;       // partials per vector, candidates per slice (vector regime)
};

__device__ __forceinline__ bool selectable(const uint32_t f) {
    return (f & FX_FLAG_SELECTABLE) && !(f & (FX_FLAG_COLLISION | FX_FLAG_BOUNDARY));
}

// grid = (tiles of 256 candidates, chunks of d.vec_chunk vectors)
template <bool REDUCE>
__global__ __launch_bounds__(FX_RESCORE_TILE) void fx_rescore_lane_kernel(const double *__restrict__ costmap, const uint32_t *__restrict__ flags,
                                                                          const double *__restrict__ w, const Dims d,
                                                                          double *__restrict__ part_cost, long long *__restrict__ part_idx,
                                                                          double *__restrict__ totals) {
    __shared__ double sc[FX_RESCORE_CHUNK_MAX][FX_RESCORE_TILE / 64];
    __shared__ long long si[FX_RESCORE_CHUNK_MAX][FX_RESCORE_TILE / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = (int64_t)blockIdx.x * FX_RESCORE_TILE + tid;
    const bool in = c < d.n;
    const uint32_t f = in ? flags[c] : 0u;
    double raw[FX_NUM_COSTS];
#pragma unroll
    for (int m = 0; m < FX_NUM_COSTS; m++) raw[m] = (in && m < d.n_cost) ? costmap[(size_t)m * d.ld + c] : 0.0;
    const bool costed = (f & FX_FLAG_COSTED) != 0, pool = in && selectable(f);
    const int v0 = (int)blockIdx.y * d.vec_chunk, v1 = min(d.n_vec, v0 + d.vec_chunk);
    for (int v = v0; v < v1; v++) {
        const double *__restrict__ wv = w + (size_t)v * d.n_cost;   // (wave-uniform)
        FxCostSum s;
#pragma unroll
        for (int m = 0; m < FX_NUM_COSTS; m++)
            if (m < d.n_cost) s = fx_cost_sum_add(d, s, m, wv[m], raw[m]);
        const double total = costed ? fx_cost_sum_close(d, s) : (double)NAN;
        if (totals && in) totals[(size_t)v * d.n + c] = total;
        if (REDUCE) {
            const bool eligible = pool && total == total;
            double bc = eligible ? total : INFINITY;
            long long bi = eligible ? (long long)c : FX_LEX_NONE;
            fx_lex_wave_min(bc, bi);
            if (lane == 0) { sc[v - v0][wave] = bc; si[v - v0][wave] = bi; }
        }
    }
    if (REDUCE) {
        __syncthreads();
        if (tid < v1 - v0) {
            double bc = sc[tid][0];
            long long bi = si[tid][0];
            for (int q = 1; q < FX_RESCORE_TILE / 64; q++)
                if (fx_lex_less(sc[tid][q], si[tid][q], bc, bi)) { bc = sc[tid][q]; bi = si[tid][q]; }
            part_cost[(size_t)(v0 + tid) * d.n_part + blockIdx.x] = bc;
            part_idx[(size_t)(v0 + tid) * d.n_part + blockIdx.x] = bi;
        }
    }
}

// grid = (slices of d.per candidates, groups of 64 vectors), one wave each
__global__ __launch_bounds__(64) void fx_rescore_vector_kernel(const double *__restrict__ costmap, const uint32_t *__restrict__ flags,
                                                               const double *__restrict__ w, const Dims d, double *__restrict__ part_cost,
                                                               long long *__restrict__ part_idx) {
    const int v = (int)blockIdx.y * 64 + (int)threadIdx.x;
    const bool live = v < d.n_vec;
    double wl[FX_NUM_COSTS];
#pragma unroll
    for (int m = 0; m < FX_NUM_COSTS; m++) wl[m] = (live && m < d.n_cost) ? w[(size_t)v * d.n_cost + m] : 0.0;
    const int64_t c0 = min(d.n, (int64_t)blockIdx.x * d.per), c1 = min(d.n, c0 + d.per);
    double bc = INFINITY;
    long long bi = FX_LEX_NONE;
    for (int64_t c = c0; c < c1; c++) {
        const uint32_t f = flags[c];                                   // (wave-uniform, as the rows below)
        if (!(f & FX_FLAG_COSTED) || !selectable(f)) continue;        // (a total without FX_FLAG_COSTED is NaN: skipped either way)
        FxCostSum s;
#pragma unroll
        for (int m = 0; m < FX_NUM_COSTS; m++)
            if (m < d.n_cost) s = fx_cost_sum_add(d, s, m, wl[m], costmap[(size_t)m * d.ld + c]);
        const double total = fx_cost_sum_close(d, s);
        // the first comparable total of the slice, then only a strictly lower one: the lower index keeps a tie (+inf included)
        if (total == total && (bi == FX_LEX_NONE || total < bc)) { bc = total; bi = (long long)c; }
    }
    if (live) {
        part_cost[(size_t)v * d.n_part + blockIdx.x] = bc;
        part_idx[(size_t)v * d.n_part + blockIdx.x] = bi;
    }
}

// grid = ceil(n_vec / 4) workgroups of four waves, a wave per vector: its partials in a strided scan, then the wave's reduction
__global__ __launch_bounds__(256) void fx_rescore_finish_kernel(const double *__restrict__ part_cost, const long long *__restrict__ part_idx,
                                                                const int64_t n_part, const int32_t n_vec, long long *__restrict__ winner,
                                                                double *__restrict__ cost) {
    const int lane = threadIdx.x & 63;
    const int v = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (v >= n_vec) return;   // (wave-uniform; no barrier below)
    double bc = INFINITY;
    long long bi = FX_LEX_NONE;
    for (int64_t p = lane; p < n_part; p += 64) {
        const double pc = part_cost[(size_t)v * n_part + p];
        const long long pi = part_idx[(size_t)v * n_part + p];
        if (fx_lex_less(pc, pi, bc, bi)) { bc = pc; bi = pi; }
    }
    fx_lex_wave_min(bc, bi);
    if (lane == 0) {
        const bool none = bi == FX_LEX_NONE;
        winner[v] = none ? -1LL : bi;
        cost[v] = none ? (double)INFINITY : bc;
    }
}

}  // namespace fxrs
