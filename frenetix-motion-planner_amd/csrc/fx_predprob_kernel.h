// fx_predprob_kernel.h -- the collision probability as the prediction cost (get_collision_probability_fast,
// collision_probability.py:141-261, summed as prediction_costs does in its commented-out branch, partial_cost_functions.py:344-356)
// over candidates of the last plan step, beside the step: nothing a step wrote is rewritten.  DESIGN.md section 16.
//
// The probability of one (obstacle, ego step) is fxrisk::step_probability in FX_RISK_PROB_MVN mode on the host's records
// (fx_risk_kernel.h, fx_api_risk.hip build_records) -- that code is included and called, not restated.
//
// Decomposition.  The K (S - 1) records of a candidate are spread over (tile of 64 listed candidates) x (chunk of steps) x
// obstacle, as the risk items of fx_risk_kernel.h are: one wave per item, grid = (tiles, chunks, K).  Obstacle and step
// are wave-uniform, so are the record and the |rho| branch of the bivariate normal; only the 5 m gate diverges, and an item none
// of whose lanes passes it costs three distances per step.
//
// Summation.  The per-obstacle sum is Sum_i p(k, i) in step order, the cost Sum_k of those in prediction order (np.sum per key,
// then += in dict order).  Floating-point addition is not associative: per-chunk partial sums added in chunk order give other
// bits for another chunk size.  An item therefore hands over the probability of EVERY step of its chunk -- the partial sums of
// one-step pieces -- into step [K][S - 1][nb] (512 contiguous bytes per wave and step), and fx_predprob_finish_kernel adds them
// in the fixed (obstacle, step) order: the same bits on every run and for every chunk size, no atomics.  The chunk size only
// decides how many waves a call has.
//
// fx_predprob_finish_kernel also re-sums the step's weighted cost from its raw cost rows (FX_MODE_WRITE_COSTMAP) with the
// prediction entry replaced, in the order and with the operations of finish_candidate (fx_eval_kernel.h) or, for a step whose
// obstacle stage ran as its own kernel, of fx_obstacle_kernel.h; fx_predprob_argmin_kernel is the lexicographic (total, index)
// minimum over the selectable collision-free candidates (fx_select.h helpers, as fx_risk_cost_argmin_kernel).
//
// Several agents in one call: the fx_predprob_batch_* kernels at the end read a table of rows in device
// memory (PredProbRow, fx_risk_args.h) where the kernels above get one agent's PredProbArgs by value -- the same items over a flat
// index, the same sums (finish_body) and the same arg-min (argmin_body), so the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_cost_sum.h"
#include "fx_risk_kernel.h"

namespace fxpp {

// One wave per (tile, chunk, obstacle): lanes = candidates j0 + 64 tile + lane of the batch [j0, j0 + nb), steps
// 1 + chunk * cs ... of obstacle blockIdx.z.  Writes step[(k (S - 1) + i - 1) nb + jj] for every step of the chunk.
__global__ __launch_bounds__(64) void fx_predprob_item_kernel(const PredProbArgs a, const int64_t j0, const int cs) {
    const int lane = threadIdx.x;
    const int k = blockIdx.z, S = a.S;
    const int64_t jj = (int64_t)blockIdx.x * 64 + lane;
    const int64_t j = j0 + jj;
    const bool in = jj < a.nb && j < a.n;
    const int64_t c = in ? (a.ids ? a.ids[j] : j) : 0;
    // ids == null: the candidates without a cost get NaN rows from the finish kernel, their probabilities are never read
    const bool live = in && (a.ids || (a.flags[c] & FX_FLAG_COSTED));
    const int i_a = 1 + (int)blockIdx.y * cs, i_b = min(S, i_a + cs);
    FxRiskParams p;   // only these three are read in MVN mode (fx_risk_kernel.h step_probability)
    p.prob_mode = FX_RISK_PROB_MVN;
    p.ego_length = a.ego_length;
    p.ego_width = a.ego_width;
    const size_t ps = (size_t)S * a.ld;
    const double *__restrict__ X = a.planes + c, *__restrict__ Y = X + ps, *__restrict__ TH = Y + ps;
    double *__restrict__ out = a.step + ((size_t)k * (S - 1)) * a.nb + jj;
    for (int i = i_a; i < i_b; i++) {
        const double *__restrict__ q = a.rec + ((size_t)k * S + i) * FXR_STRIDE;
        double pr = 0.0;
        if (live) pr = fxrisk::step_probability(p, q, X[(size_t)i * a.ld], Y[(size_t)i * a.ld], TH[(size_t)i * a.ld]);
        if (jj < a.nb) out[(size_t)(i - 1) * a.nb] = pr;
    }
}

// One lane per candidate of the batch: the sums in (obstacle, step) order, the re-sum of the step's cost
__device__ __forceinline__ void finish_body(const PredProbArgs &a, const int64_t j0, const int64_t jj) {
    const int64_t j = j0 + jj;
    if (jj >= a.nb || j >= a.n) return;
    const size_t n = (size_t)a.n;
    const int64_t c = a.ids ? a.ids[j] : j;
    const int K = a.K, S = a.S;
    if (!a.ids && !(a.flags[c] & FX_FLAG_COSTED)) {
        a.prob[j] = NAN;
        a.total[j] = NAN;
        if (a.prob_obs)
            for (int k = 0; k < K; k++) a.prob_obs[(size_t)k * n + j] = NAN;
        return;
    }
    double pred = 0.0;
    if (a.source == FX_PRED_SOURCE_PROBABILITY) {
        for (int k = 0; k < K; k++) {
            const double *__restrict__ sp = a.step + ((size_t)k * (S - 1)) * a.nb + jj;
            double s = 0.0;
            for (int i = 0; i < S - 1; i++) s += sp[(size_t)i * a.nb];
            if (a.prob_obs) a.prob_obs[(size_t)k * n + j] = s;
            pred += s;
        }
    } else {
        pred = a.costmap[(size_t)a.n_pred * a.ld + c];
        if (a.prob_obs)
            for (int k = 0; k < K; k++) a.prob_obs[(size_t)k * n + j] = NAN;   // (the step keeps no per-obstacle sums)
    }
    // weighted sum in the cost list's order (fx_eval_kernel.h finish_candidate): sum = -0.0; sum += w * c per term;
    // total = 0.0 + sum.  A deferred step (fx_obstacle_kernel.h) added the terms behind the prediction as ONE addend, tail
    // (fx_cost_sum.h: the sum the re-score kernels share).
    FxCostSum s;
    for (int m = 0; m < a.n_cost; m++) {
        const double cm = m == a.n_pred ? pred : a.costmap[(size_t)m * a.ld + c];
        s = fx_cost_sum_add(a, s, m, a.cost_w[m], cm);
    }
    s = fx_cost_sum_join(a, s);
    a.prob[j] = pred;
    a.total[j] = fx_cost_sum_total(s);
}
__global__ __launch_bounds__(256) void fx_predprob_finish_kernel(const PredProbArgs a, const int64_t j0) {
    finish_body(a, j0, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// (total, index) minimum over the listed candidates with FX_FLAG_SELECTABLE and neither FX_FLAG_COLLISION nor FX_FLAG_BOUNDARY,
// NaN skipped, -1 when nothing is left: ONE workgroup of 1024 lanes; out[0] = index, out[1] = the cost's bits
__device__ __forceinline__ void argmin_body(const double *__restrict__ total, int64_t n, const int64_t *__restrict__ ids,
                                            const uint32_t *__restrict__ flags, long long *__restrict__ out) {
    double bc;
    long long bi;
    fx_lex_block_min(n, ids, [=](int64_t j, long long c, double &t) {
        const uint32_t f = flags[c];
        t = total[j];
        return (f & FX_FLAG_SELECTABLE) && !(f & (FX_FLAG_COLLISION | FX_FLAG_BOUNDARY)) && t == t;
    }, bc, bi);
    if (threadIdx.x == 0) {
        const bool none = bi == FX_LEX_NONE;
        out[0] = none ? -1LL : bi;
        out[1] = __double_as_longlong(none ? (double)NAN : bc);
    }
}
__global__ __launch_bounds__(1024) void fx_predprob_argmin_kernel(const double *__restrict__ total, int64_t n,
                                                                  const int64_t *__restrict__ ids, const uint32_t *__restrict__ flags,
                                                                  long long *__restrict__ out) {
    argmin_body(total, n, ids, flags, out);
}

// ---- several agents in one call (fx_eval_prediction_prob_batch) ----
// The row of flat index `at` (an item of the item launch, a workgroup of the finish launch) among the n_rows rows of a round, whose
// first indices `first0` ascend: the last row that starts at or before `at`.  Rows without an item share their first index with
// the row behind them, which is the one found.  One load per 64 rows and a ballot: `at` is wave-uniform, so is the answer.
template <typename T>
__device__ __forceinline__ int row_of(const T *__restrict__ first0, const int n_rows, const int64_t at) {
    const int lane = threadIdx.x & 63;
    int r = 0;
    for (int b = 0; b < n_rows; b += 64) r += __popcll(__ballot(b + lane < n_rows && (int64_t)first0[b + lane] <= at));
    return __builtin_amdgcn_readfirstlane(r - 1);
}

// One wave per item of a round: grid.x = the round's items exactly, so no workgroup exists for an (agent, chunk, obstacle) that
// does not.  rows, item0: of the round.
__global__ __launch_bounds__(64) void fx_predprob_batch_item_kernel(const PredProbRow *__restrict__ rows, const int64_t *__restrict__ item0,
                                                                    const int n_rows) {
    const int64_t at = blockIdx.x;
    const PredProbRow &r = rows[row_of(item0, n_rows, at)];
    const PredProbArgs &a = r.a;
    // tile, chunk and obstacle of the item, wave-uniform; from here on the loop of fx_predprob_item_kernel with ids == null (its
    // own text: sharing it moved that kernel's register allocation, and it is to stay what it was -- DESIGN.md section 18)
    const int64_t local = at - r.item0, tiles = a.nb / 64, rest = local / tiles;
    const int lane = threadIdx.x, S = a.S, cs = r.cs;
    const int k = (int)(rest / r.chunks);
    const int64_t jj = (local % tiles) * 64 + lane;
    const int64_t c = r.first + jj;
    const bool live = jj < a.nb && c < a.n && (a.flags[c < a.n ? c : 0] & FX_FLAG_COSTED);
    const int i_a = 1 + (int)(rest % r.chunks) * cs, i_b = min(S, i_a + cs);
    FxRiskParams p;   // only these three are read in MVN mode (fx_risk_kernel.h step_probability)
    p.prob_mode = FX_RISK_PROB_MVN;
    p.ego_length = a.ego_length;
    p.ego_width = a.ego_width;
    const size_t ps = (size_t)S * a.ld;
    const double *__restrict__ X = a.planes + (live ? c : 0), *__restrict__ Y = X + ps, *__restrict__ TH = Y + ps;
    double *__restrict__ out = a.step + ((size_t)k * (S - 1)) * a.nb + jj;
    for (int i = i_a; i < i_b; i++) {
        const double *__restrict__ q = a.rec + ((size_t)k * S + i) * FXR_STRIDE;
        double pr = 0.0;
        if (live) pr = fxrisk::step_probability(p, q, X[(size_t)i * a.ld], Y[(size_t)i * a.ld], TH[(size_t)i * a.ld]);
        if (jj < a.nb) out[(size_t)(i - 1) * a.nb] = pr;
    }
}

// One lane per (agent, candidate) of a round: grid.x = the rows' workgroups of 256
__global__ __launch_bounds__(256) void fx_predprob_batch_finish_kernel(const PredProbRow *__restrict__ rows, const int32_t *__restrict__ fin0,
                                                                       const int n_rows) {
    const PredProbRow &r = rows[row_of(fin0, n_rows, (int64_t)blockIdx.x)];
    const int64_t jj = (int64_t)(blockIdx.x - r.fin0) * blockDim.x + threadIdx.x;
    if (jj < r.count) finish_body(r.a, r.first, jj);
}

// One workgroup of 1024 lanes per listed agent: out[2 agent] = index, out[2 agent + 1] = the cost's bits
__global__ __launch_bounds__(1024) void fx_predprob_batch_argmin_kernel(const PredProbRow *__restrict__ rows,
                                                                        const int32_t *__restrict__ agent_row, long long *__restrict__ out) {
    const int row = agent_row[blockIdx.x];
    if (row < 0) {   // (an agent without a candidate)
        if (threadIdx.x == 0) { out[2 * blockIdx.x] = -1LL; out[2 * blockIdx.x + 1] = __double_as_longlong((double)NAN); }
        return;
    }
    const PredProbArgs &a = rows[row].a;
    argmin_body(a.total, a.n, nullptr, a.flags, out + 2 * blockIdx.x);
}

}  // namespace fxpp
