// fx_rescore_batch_kernel.h -- the re-score of fx_rescore_kernel.h for a table of ENTRIES in one call, over effective cost lists
// (host: fx_api_rescore.hip; table: fx_rescore_batch_plan.h).
//
// An entry is one agent with its own weight vectors.  Its effective list is the step's own cost list with up to two rows from
// outside the step: one given in place of the prediction's row, one more term (the responsibility).  The kernels read a candidate's
// values through the entry's table of row base pointers and know nothing of which term is which: total(c) is FxCostSum
// (fx_cost_sum.h) over the effective list, with n_cost its length and n_pred the prediction's position in it.
//
// The entries of a regime share one launch with a flat 1-D grid; a workgroup finds its entry with the ballot search of the other
// batched passes (fxrisk::batch_row_of) over the entries' first workgroups, then tile and chunk (slice and group) by division --
// from there on the loops of fx_rescore_kernel.h in their own text (those kernels stay what they are), the partials in the same
// layout [n_vec][n_part] of the entry's own plan.  So every result carries the bits of the per-agent call.  FP64, no atomics.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_cost_sum.h"
#include "fx_rescore_batch_plan.h"
#include "fx_rescore_kernel.h"
#include "fx_risk_kernel.h"
#include "fx_select.h"

namespace fxrs {

// grid = all workgroups of the table's entries: per entry (tiles of 256 candidates) x (chunks of e.vec_chunk vectors)
template <bool REDUCE>
__global__ __launch_bounds__(FX_RESCORE_TILE) void fx_rescore_batch_lane_kernel(const FxRescoreEntry *__restrict__ entries,
                                                                                const int64_t *__restrict__ wg0, const int n_entries) {
    __shared__ double sc[FX_RESCORE_CHUNK_MAX][FX_RESCORE_TILE / 64];
    __shared__ long long si[FX_RESCORE_CHUNK_MAX][FX_RESCORE_TILE / 64];
    const FxRescoreEntry &e = entries[fxrisk::batch_row_of(wg0, n_entries, (int64_t)blockIdx.x)];
    const int64_t local = (int64_t)blockIdx.x - e.wg0, tile = local % e.n_part;
    const int chunk = (int)(local / e.n_part);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = tile * FX_RESCORE_TILE + tid;
    const bool in = c < e.n;
    const uint32_t f = in ? e.flags[c] : 0u;
    double raw[FX_RESCORE_ROWS];
#pragma unroll
    for (int m = 0; m < FX_RESCORE_ROWS; m++) raw[m] = (in && m < e.n_cost) ? e.row[m][c] : 0.0;
    const bool costed = (f & FX_FLAG_COSTED) != 0, pool = in && selectable(f);
    const int v0 = chunk * e.vec_chunk, v1 = min(e.n_vec, v0 + e.vec_chunk);
    double *__restrict__ totals = e.totals;
    for (int v = v0; v < v1; v++) {
        const double *__restrict__ wv = e.w + (size_t)v * e.n_cost;   // (wave-uniform)
        FxCostSum s;
#pragma unroll
        for (int m = 0; m < FX_RESCORE_ROWS; m++)
            if (m < e.n_cost) s = fx_cost_sum_add(e, s, m, wv[m], raw[m]);
        const double total = costed ? fx_cost_sum_close(e, s) : (double)NAN;
        if (totals && in) totals[(size_t)v * e.n + c] = total;
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
            e.part_cost[(size_t)(v0 + tid) * e.n_part + tile] = bc;
            e.part_idx[(size_t)(v0 + tid) * e.n_part + tile] = bi;
        }
    }
}

// grid = all waves of the table's entries: per entry (slices of e.per candidates) x (groups of 64 vectors)
__global__ __launch_bounds__(64) void fx_rescore_batch_vector_kernel(const FxRescoreEntry *__restrict__ entries, const int64_t *__restrict__ wg0,
                                                                     const int n_entries) {
    const FxRescoreEntry &e = entries[fxrisk::batch_row_of(wg0, n_entries, (int64_t)blockIdx.x)];
    const int64_t local = (int64_t)blockIdx.x - e.wg0, slice = local % e.n_part;
    const int v = (int)(local / e.n_part) * 64 + (int)threadIdx.x;
    const bool live = v < e.n_vec;
    double wl[FX_RESCORE_ROWS];
#pragma unroll
    for (int m = 0; m < FX_RESCORE_ROWS; m++) wl[m] = (live && m < e.n_cost) ? e.w[(size_t)v * e.n_cost + m] : 0.0;
    const int64_t c0 = min(e.n, slice * e.per), c1 = min(e.n, c0 + e.per);
    double bc = INFINITY;
    long long bi = FX_LEX_NONE;
    for (int64_t c = c0; c < c1; c++) {
        const uint32_t f = e.flags[c];                                 // (wave-uniform, as the rows below)
        if (!(f & FX_FLAG_COSTED) || !selectable(f)) continue;        // (a total without FX_FLAG_COSTED is NaN: skipped either way)
        FxCostSum s;
#pragma unroll
        for (int m = 0; m < FX_RESCORE_ROWS; m++)
            if (m < e.n_cost) s = fx_cost_sum_add(e, s, m, wl[m], e.row[m][c]);
        const double total = fx_cost_sum_close(e, s);
        // the first comparable total of the slice, then only a strictly lower one: the lower index keeps a tie (+inf included)
        if (total == total && (bi == FX_LEX_NONE || total < bc)) { bc = total; bi = (long long)c; }
    }
    if (live) {
        e.part_cost[(size_t)v * e.n_part + slice] = bc;
        e.part_idx[(size_t)v * e.n_part + slice] = bi;
    }
}

// grid = ceil(vectors of all entries / 4) workgroups of four waves, a wave per (entry, vector): fin0 [n_entries] the entries' first waves
__global__ __launch_bounds__(256) void fx_rescore_batch_finish_kernel(const FxRescoreEntry *__restrict__ entries, const int64_t *__restrict__ fin0,
                                                                      const int n_entries, const int64_t n_waves) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (int64_t)(threadIdx.x >> 6);
    if (g >= n_waves) return;   // (wave-uniform; no barrier below)
    const FxRescoreEntry &e = entries[fxrisk::batch_row_of(fin0, n_entries, g)];
    const int64_t v = g - e.fin0, n_part = e.n_part;
    double bc = INFINITY;
    long long bi = FX_LEX_NONE;
    for (int64_t p = lane; p < n_part; p += 64) {
        const double pc = e.part_cost[(size_t)v * n_part + p];
        const long long pi = e.part_idx[(size_t)v * n_part + p];
        if (fx_lex_less(pc, pi, bc, bi)) { bc = pc; bi = pi; }
    }
    fx_lex_wave_min(bc, bi);
    if (lane == 0) {
        const bool none = bi == FX_LEX_NONE;
        e.winner[v] = none ? -1LL : bi;
        e.cost[v] = none ? (double)INFINITY : bc;
    }
}

}  // namespace fxrs
