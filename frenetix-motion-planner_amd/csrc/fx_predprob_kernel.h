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
#pragma once

#include <hip/hip_runtime.h>

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
__global__ __launch_bounds__(256) void fx_predprob_finish_kernel(const PredProbArgs a, const int64_t j0) {
    const int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
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
    // total = 0.0 + sum.  A deferred step (fx_obstacle_kernel.h) added the terms behind the prediction as ONE addend, tail.
    double sum = -0.0, tail = 0.0;
    for (int m = 0; m < a.n_cost; m++) {
        const double cm = m == a.n_pred ? pred : a.costmap[(size_t)m * a.ld + c];
        const double t = a.cost_w[m] * cm;
        if (a.deferred && m > a.n_pred) tail += t;
        else sum += t;
    }
    if (a.deferred && a.n_pred + 1 < a.n_cost) sum += tail;
    a.prob[j] = pred;
    a.total[j] = 0.0 + sum;
}

// (total, index) minimum over the listed candidates with FX_FLAG_SELECTABLE and neither FX_FLAG_COLLISION nor FX_FLAG_BOUNDARY,
// NaN skipped, -1 when nothing is left: ONE workgroup of 1024 lanes; out[0] = index, out[1] = the cost's bits
__global__ __launch_bounds__(1024) void fx_predprob_argmin_kernel(const double *__restrict__ total, int64_t n,
                                                                  const int64_t *__restrict__ ids, const uint32_t *__restrict__ flags,
                                                                  long long *__restrict__ out) {
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

}  // namespace fxpp
