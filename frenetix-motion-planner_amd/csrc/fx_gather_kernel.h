// fx_gather_kernel.h -- batched candidate read-back (fx_read_candidates_agent): for a list of n candidate
// indices of one agent, one packed record per listed candidate, in the caller's order (unsorted lists and duplicates are legal):
//   planes[FX_NUM_PLANES][S] | lon[6] lat[6] tau_lat | raw_costs[n_cost] | cost | traj_len | flags | boundary_step
// gathered from the structure-of-arrays outputs of the last step into a device buffer that ONE copy brings to the host -- what
// the reference's adapter does per object (reactive_planner_cpp.py:353-358) and the planner for the trajectories it keeps
// (:430, 437).
//
// The kernel runs behind the step on the context's stream: a kernel boundary lies between the writers and these loads, so they
// are plain global loads.  It writes only its own output buffer, takes no atomics, no tickets and waits for nothing: it cannot
// hang.  One workgroup per record; lane q of the workgroup owns words q, q + 256, ... of the record: every source word sits in
// its own 64-byte line (stride ld * 8 B) unless neighbouring indices are listed too -- the host sorts the list, so that
// neighbouring workgroups touch neighbouring lines while they are hot in L2 -- and the record's stores are contiguous.  A lane
// requests FX_GATHER_UNROLL words before its first store (1 024 words per round of the workgroup: S <= 70 in one round).
#pragma once
#include "fx_device.h"

#define FX_GATHER_BLOCK 256
#define FX_GATHER_UNROLL 4

// source of word q < n_dbl of candidate l's record -- the 8-byte sources: planes, coefficients, raw costs, cost -- and whether the step
// produced it.  The lane picks an ADDRESS, the caller does one load (a load behind each branch would be a round trip per branch:
// fx_tail.h).
__device__ __forceinline__ const FX_GLOBAL unsigned long long *fx_gather_source(const GatherArgs &a, int64_t l, int q, int n_pl, int n_dbl,
                                                                               bool *have) {
    const FX_GLOBAL double *src = as_global(a.planes) + (size_t)q * a.ld;
    bool h = (a.parts & FX_GATHER_BUNDLE) != 0;
    if (q >= n_pl) src = as_global(a.coeffs) + (size_t)(q - n_pl) * a.ld;
    if (q >= n_pl + FX_COEFF_ROWS) { src = as_global(a.costmap) + (size_t)(q - n_pl - FX_COEFF_ROWS) * a.ld; h = (a.parts & FX_GATHER_COSTMAP) != 0; }
    if (q >= n_dbl - 1) { src = as_global(a.cost); h = true; }
    *have = h;
    return reinterpret_cast<const FX_GLOBAL unsigned long long *>(src + l);
}

__global__ __launch_bounds__(FX_GATHER_BLOCK) void fx_gather_candidates_kernel(const GatherArgs a, const int64_t *__restrict__ ids, int64_t n,
                                                                              unsigned long long *__restrict__ out) {
    const int64_t rec = blockIdx.x;
    if (rec >= n) return;
    const int n_pl = FX_NUM_PLANES * a.S;
    const int n_dbl = n_pl + FX_COEFF_ROWS + a.n_cost + 1;
    const int W = FX_GATHER_WORDS(a.S, a.n_cost);   // = n_dbl + 3: traj_len | flags | boundary_step
    const int64_t l = ids[rec];
    const bool ok = l >= 0 && l < a.C;   // (the host has validated the list; an index outside the agent is never dereferenced)
    unsigned long long *o = out + (size_t)rec * W;
    // the three integer words, by the last three lanes (the 8-byte words start at lane 0)
    const int j = (int)threadIdx.x - (FX_GATHER_BLOCK - 3);
    unsigned long long iw = 0ULL;
    if (ok && j == 0 && (a.parts & FX_GATHER_BUNDLE)) iw = (unsigned long long)(long long)as_global(a.traj_len)[l];
    if (ok && j == 1) iw = (unsigned long long)as_global(a.flags)[l];
    if (ok && j == 2 && (a.parts & FX_GATHER_BOUNDARY)) iw = (unsigned long long)(long long)as_global(a.bound_step)[l];
    for (int q0 = (int)threadIdx.x; q0 < n_dbl; q0 += FX_GATHER_BLOCK * FX_GATHER_UNROLL) {
        unsigned long long v[FX_GATHER_UNROLL];
#pragma unroll
        for (int u = 0; u < FX_GATHER_UNROLL; u++) {
            const int q = q0 + u * FX_GATHER_BLOCK;
            bool have;
            const FX_GLOBAL unsigned long long *src = fx_gather_source(a, l, q < n_dbl ? q : 0, n_pl, n_dbl, &have);
            v[u] = (ok && have && q < n_dbl) ? *src : 0ULL;
        }
#pragma unroll
        for (int u = 0; u < FX_GATHER_UNROLL; u++) {
            const int q = q0 + u * FX_GATHER_BLOCK;
            if (q < n_dbl) o[q] = v[u];
        }
    }
    if (j >= 0) o[n_dbl + j] = iw;
}
