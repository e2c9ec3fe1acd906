// fx_risk_items_kernel.h -- the trajectory-risk walk of fx_risk_kernel.h in the item decomposition of fx_predprob_kernel.h, and the
// responsibility cost as a weighted term of the step's cost sum beside the step.  DESIGN.md section 17.
//
// Decomposition.  risk_walk gives one lane the serial chain of all K (S - 1) (obstacle, step) pairs.  Here the pairs are spread over
// (tile of 64 listed candidates) x (chunk of steps) x obstacle: one wave per item, grid = (tiles, chunks, K).  Obstacle and step
// are wave-uniform, so are the record, the prediction and the |rho| branch; only the 5 m gate diverges.  The probability of a step
// is fxrisk::step_probability and the harm fxrisk::step_harm -- included and called, what risk_walk calls.
//
// Why the results are risk_walk's bit for bit.  Every per-step value is computed by the same function on the same operands
// (-ffp-contract=off: no fused operation may differ between two inlined copies).  Everything the walk keeps of them is a maximum
// taken with fmax from -inf -- associative and commutative bit for bit, NaN operands dropped on either side -- or the FIRST maximum
// of the probability list with the harm that stands beside it (strict >): a chunk keeps its first maximum, and the chunks, combined
// in chunk order with the same strict >, keep the first of those.  p_nan is an OR.  So the chunk size decides how many waves a
// call has and nothing else, and no atomics are needed: an item owns its partials.
//
// Partials.  part [K][chunks][NV][nb] of one batch of nb candidates, candidate innermost: a wave stores 512 contiguous bytes per
// value.  NV = 2 (plain pass: e_max, o_max) or 7 (detail: + he_max, ho_max, p_max, ho_at, p_nan as 0 / 1).  An item whose chunk
// begins at or behind pl = min(S - 1, npos) of its obstacle ends at once and writes nothing; the finish kernel reads the
// ceil(pl / cs) chunks that ran.
//
// Parameters.  FxRiskParams comes through a pointer into the pass's device block, not by value as the walk takes it: the bins of
// angle_coef then are scalar loads at wave-uniform addresses.  By value the structure gets a private copy -- 280 bytes of scratch
// per lane and one wave per SIMD, as the walk has; through the pointer the item kernel has no scratch and two waves per SIMD.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_risk_kernel.h"

namespace fxri {

enum { P_EMAX = 0, P_OMAX = 1, P_HEMAX = 2, P_HOMAX = 3, P_PMAX = 4, P_HOAT = 5, P_PNAN = 6 };

// a candidate of the batch that the pass evaluates: listed, or -- every candidate -- with all of it.need in its flags
__device__ __forceinline__ bool selected(const RiskWalkArgs &w, const RiskItemArgs &it, int64_t c) {
    return w.ids || (w.flags[c] & it.need) == it.need;
}

// One wave per (tile, chunk, obstacle): lanes = candidates j0 + 64 tile + lane of the batch [j0, j0 + nb), steps t = chunk cs ...
// of obstacle blockIdx.z.  DETAIL as in risk_walk: the harm at every step, and the four further partials.
template <bool DETAIL>
__global__ __launch_bounds__(64) void fx_risk_item_kernel(const RiskWalkArgs w, const RiskItemArgs it, const int64_t j0) {
    const int lane = threadIdx.x;
    const FxRiskParams &p = *it.params;
    const int k = blockIdx.z, S = w.S, NV = DETAIL ? 7 : 2;
    const double *__restrict__ o = w.obs + (size_t)k * FXO_STRIDE;
    const int pl = min(S - 1, (int)o[FXO_NPOS]);
    const int t_a = (int)blockIdx.y * it.cs, t_b = min(pl, t_a + it.cs);
    if (t_a >= t_b) return;   // (wave-uniform)
    const int64_t jj = (int64_t)blockIdx.x * 64 + lane;
    const int64_t j = j0 + jj;
    if (jj >= it.nb || j >= w.n) return;
    const int64_t c = w.ids ? w.ids[j] : j;
    if (!selected(w, it, c)) return;   // (NaN rows from the finish kernel)
    const int64_t ld = w.ld;
    const double *__restrict__ X = w.planes + c, *__restrict__ Y = X + (size_t)S * ld, *__restrict__ TH = Y + (size_t)S * ld,
                 *__restrict__ V = TH + (size_t)S * ld;
    const bool prot = o[FXO_CLS] == (double)FX_RISK_CLASS_PROTECTED;
    const double me = p.ego_mass, mo = o[FXO_MASS];
    const double f_ego = mo / (me + mo), f_obs = me / (me + mo);
    double e_max = -INFINITY, o_max = -INFINITY;
    double he_max = -INFINITY, ho_max = -INFINITY, p_max = -INFINITY, ho_at = 0.0;   // DETAIL
    bool p_nan = false;
    for (int t = t_a; t < t_b; t++) {
        const int i = t + 1;
        const double *__restrict__ q = w.rec + ((size_t)k * S + i) * FXR_STRIDE;
        const double prob = fxrisk::step_probability(p, q, X[(size_t)i * ld], Y[(size_t)i * ld], TH[(size_t)i * ld]);
        double re = 0.0, ro = 0.0;
        if (DETAIL || prob != 0.0) {
            const size_t kt = (size_t)k * w.P + t;
            double he, ho;
            fxrisk::step_harm(p, prot, f_ego, f_obs, X[(size_t)t * ld], Y[(size_t)t * ld], TH[(size_t)t * ld], V[(size_t)t * ld], w.yaw[kt],
                              w.vo[kt], w.pos[2 * kt], w.pos[2 * kt + 1], he, ho);
            re = prob != 0.0 ? he * prob : 0.0;
            ro = prob != 0.0 ? ho * prob : 0.0;
            if (DETAIL) {
                he_max = fmax(he_max, he);
                ho_max = fmax(ho_max, ho);
                p_nan = p_nan || prob != prob;
                if (prob > p_max) { p_max = prob; ho_at = ho; }
            }
        }
        e_max = fmax(e_max, re);
        o_max = fmax(o_max, ro);
    }
    double *__restrict__ out = it.part + (((size_t)k * it.chunks + blockIdx.y) * NV) * (size_t)it.nb + jj;
    out[(size_t)P_EMAX * it.nb] = e_max;
    out[(size_t)P_OMAX * it.nb] = o_max;
    if (DETAIL) {
        out[(size_t)P_HEMAX * it.nb] = he_max;
        out[(size_t)P_HOMAX * it.nb] = ho_max;
        out[(size_t)P_PMAX * it.nb] = p_max;
        out[(size_t)P_HOAT * it.nb] = ho_at;
        out[(size_t)P_PNAN * it.nb] = p_nan ? 1.0 : 0.0;
    }
}

// One lane per candidate of the batch: per obstacle the chunks in chunk order, then what risk_walk writes behind its step loop
template <bool DETAIL>
__global__ __launch_bounds__(256) void fx_risk_items_finish_kernel(const RiskWalkArgs w, const RiskItemArgs it, const int64_t j0,
                                                                  double *__restrict__ out_ego, double *__restrict__ out_obst,
                                                                  double *__restrict__ col, double *__restrict__ out_occ) {
    const int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = j0 + jj;
    if (jj >= it.nb || j >= w.n) return;
    const size_t n = (size_t)w.n, nb = (size_t)it.nb;
    const int K = w.K, S = w.S, NV = DETAIL ? 7 : 2;
    const int64_t c = w.ids ? w.ids[j] : j;
    if (!selected(w, it, c)) {
        out_ego[j] = NAN;
        out_obst[j] = NAN;
        if (DETAIL) {
            out_occ[j] = NAN;
            for (int q = 0; q < 4 * K; q++) col[(size_t)q * n + j] = NAN;
        }
        return;
    }
    double ego_best = -INFINITY, obst_best = -INFINITY, occ_best = -INFINITY;
    bool any = false;
    for (int k = 0; k < K; k++) {
        const int pl = min(S - 1, (int)w.obs[(size_t)k * FXO_STRIDE + FXO_NPOS]);
        if (pl <= 0) {
            if (DETAIL)
                for (int q = 0; q < 4; q++) col[((size_t)q * K + k) * n + j] = 0.0;
            continue;
        }
        const int nch = (pl + it.cs - 1) / it.cs;
        double e_max = -INFINITY, o_max = -INFINITY;
        double he_max = -INFINITY, ho_max = -INFINITY, p_max = -INFINITY, ho_at = 0.0;
        bool p_nan = false;
        for (int ch = 0; ch < nch; ch++) {
            const double *__restrict__ in = it.part + (((size_t)k * it.chunks + ch) * NV) * nb + jj;
            e_max = fmax(e_max, in[(size_t)P_EMAX * nb]);
            o_max = fmax(o_max, in[(size_t)P_OMAX * nb]);
            if (DETAIL) {
                he_max = fmax(he_max, in[(size_t)P_HEMAX * nb]);
                ho_max = fmax(ho_max, in[(size_t)P_HOMAX * nb]);
                p_nan = p_nan || in[(size_t)P_PNAN * nb] != 0.0;
                const double pm = in[(size_t)P_PMAX * nb];
                if (pm > p_max) { p_max = pm; ho_at = in[(size_t)P_HOAT * nb]; }
            }
        }
        ego_best = fmax(ego_best, e_max);
        obst_best = fmax(obst_best, o_max);
        any = true;
        if (DETAIL) {
            col[((size_t)0 * K + k) * n + j] = e_max;
            col[((size_t)1 * K + k) * n + j] = o_max;
            col[((size_t)2 * K + k) * n + j] = he_max;
            col[((size_t)3 * K + k) * n + j] = ho_max;
            occ_best = fmax(occ_best, (!p_nan && p_max > 0.001) ? ho_at : 0.0);   // risk_costs.py:104-107
        }
    }
    out_ego[j] = any ? ego_best : 0.0;
    out_obst[j] = any ? obst_best : 0.0;
    if (DETAIL) out_occ[j] = any ? occ_best : 0.0;
}

// The responsibility cost as one more weighted term of the step's cost sum: one lane per listed candidate re-sums the step's raw
// cost rows (FX_MODE_WRITE_COSTMAP) with w_resp * resp inserted in front of entry a.at -- its place in the name-sorted list,
// between `prediction` and `velocity_offset` -- in the order and with the operations of fx_predprob_finish_kernel: sum = -0.0;
// sum += w * c per term; a deferred step (fx_obstacle_kernel.h) added the terms behind the prediction as ONE addend, which the new
// term then joins.  The prediction entry is the step's own, or a.pred [n] (the prob of a collision-probability pass over the same
// candidates).  resp [n] is row 4 of fx_risk_cost_kernel's output.
__global__ __launch_bounds__(256) void fx_resp_finish_kernel(const RespSumArgs a) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    const int64_t c = a.ids ? a.ids[j] : j;
    if (!a.ids && (a.flags[c] & a.need) != a.need) {
        a.resp_out[j] = NAN;
        a.total[j] = NAN;
        return;
    }
    const double resp = a.resp[j];
    double sum = -0.0, tail = 0.0;
    const bool defer = a.deferred && a.n_pred >= 0;
    for (int m = 0; m <= a.n_cost; m++) {
        if (m == a.at) {
            const double t = a.w_resp * resp;
            if (defer && m > a.n_pred) tail += t;
            else sum += t;
        }
        if (m == a.n_cost) break;
        const double cm = (m == a.n_pred && a.pred) ? a.pred[j] : a.costmap[(size_t)m * a.ld + c];
        const double t = a.cost_w[m] * cm;
        if (defer && m > a.n_pred) tail += t;
        else sum += t;
    }
    if (defer) sum += tail;   // (never empty: the new term stands behind the prediction)
    a.resp_out[j] = resp;
    a.total[j] = 0.0 + sum;
}

}  // namespace fxri
