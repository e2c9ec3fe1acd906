// fx_risk_kernel.h -- trajectory risk (risk_costs.py:20-118, crash_angle_simplified) over the materialised bundle, and the
// arg-min of ego + obstacle risk (reactive_planner.py:262-269, reactive_planner_cpp.py:404-413).  DESIGN.md section 11.
// With calc_risk's per-obstacle results, the risk-cost principles with the responsibility cost over them (risk_costs.py:124-251,
// utility/responsibility.py), and the responsibility cost as a weighted term of the step's cost sum beside the
// step.  Behind them the forms of these passes for several agents in one call (DESIGN.md sections 19 - 21).
//
// Decomposition.  The K (S - 1) (obstacle, step) pairs of a candidate are spread over (tile of 64 listed candidates) x (chunk of
// steps) x obstacle: one wave per item, grid = (tiles, chunks, K), and one finish lane per candidate behind them.  Obstacle and
// step are wave-uniform, so everything indexed by them -- the three obstacle means, the standardisation (sigma_x, sigma_y, rho),
// the |rho| branch of the bivariate normal and its node terms -- comes from a record the host built once per call
// (fx_api_risk.hip; its layout, FXR_* / FXO_*, is in fx_risk_args.h).  Only the 5 m gate diverges.
//
// Why the chunk size cannot change a bit.  Everything a candidate keeps of its per-step values is a maximum taken with fmax from
// -inf -- associative and commutative bit for bit, NaN operands dropped on either side -- or the FIRST maximum of the probability
// list with the harm that stands beside it (strict >): a chunk keeps its first maximum, and the chunks, combined in chunk order
// with the same strict >, keep the first of those.  p_nan is an OR.  So the chunk size decides how many waves a call has and
// nothing else, and no atomics are needed: an item owns its partials.
//
// Partials.  part [K][chunks][NV][nb] of one batch of nb candidates, candidate innermost: a wave stores 512 contiguous bytes per
// value.  NV = 2 (plain pass: e_max, o_max) or 7 (detail: + he_max, ho_max, p_max, ho_at, p_nan as 0 / 1).  An item whose chunk
// begins at or behind pl = min(S - 1, npos) of its obstacle ends at once and writes nothing; the finish kernel reads the
// ceil(pl / cs) chunks that ran.
//
// Parameters.  FxRiskParams comes through a pointer into the pass's device block, not by value: the bins of angle_coef then are
// scalar loads at wave-uniform addresses, where a by-value structure gets a private copy -- 280 bytes of scratch per lane.
//
// Bivariate normal upper probability BVNU(h, k, rho) = P(X > h, Y > k) after Genz (2004), Statistics and Computing 14:251-260:
// Drezner-Wesolowsky Gauss-Legendre quadrature of the Plackett integral in asin(rho) with 6 / 12 / 20 nodes for |rho| < 0.3 /
// 0.75 / 0.925, and for |rho| >= 0.925 the expansion around rho = +-1 plus 20-node quadrature of the remainder.  The rectangle
// probability of `mvnun` is BVNU(a1, a2) - BVNU(b1, a2) - BVNU(a1, b2) + BVNU(b1, b2) on the standardised bounds.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_risk_args.h"
#include "fx_select.h"

namespace fxrisk {

// Gauss-Legendre weights on [-1, 1], positive half (the nodes live in the host's records)
__constant__ double kW6[3] = {0.1713244923791705, 0.3607615730481384, 0.4679139345726904};
__constant__ double kW12[6] = {0.04717533638651177, 0.1069393259953183, 0.1600783285433464,
                               0.2031674267230659, 0.2334925365383547, 0.2491470458134029};
__constant__ double kW20[10] = {0.01761400713915212, 0.04060142980038694, 0.06267204833410906, 0.08327674157670475,
                                0.1019301198172404,  0.1181945319615184,  0.1316886384491766,  0.1420961093183821,
                                0.1491729864726037,  0.1527533871307259};

__device__ __forceinline__ double phid(double z) { return 0.5 * erfc(-z / 1.4142135623730951); }

__device__ __forceinline__ double weight(int ng, int j) { return ng == 3 ? kW6[j] : (ng == 6 ? kW12[j] : kW20[j]); }

// BVNU(h, k, rho) with the wave-uniform part of rho taken from the record q
__device__ double bvnu(double h, double k, const double *__restrict__ q) {
    const double r = q[FXR_RHO];
    const int branch = (int)q[FXR_BRANCH];
    if (branch == 0) return phid(-h) * phid(-k);
    const double tp = 6.283185307179586;
    const int ng = (int)q[FXR_NG];
    double hk = h * k, bvn = 0.0;
    if (branch == 1) {
        const double hs = (h * h + k * k) / 2.0, asr = q[FXR_ASR];
        for (int j = 0; j < 2 * ng; j++) {
            const double sn = q[FXR_N1 + j];
            bvn += weight(ng, j < ng ? j : j - ng) * exp((sn * hk - hs) / (1.0 - sn * sn));
        }
        bvn = bvn * asr / tp + phid(-h) * phid(-k);
    } else {
        if (r < 0.0) { k = -k; hk = -hk; }
        if (branch == 2) {
            const double as = q[FXR_ASR], a = q[FXR_A], bs = (h - k) * (h - k);
            const double c = (4.0 - hk) / 8.0, d = (12.0 - hk) / 80.0;
            double asr = -(bs / as + hk) / 2.0;
            if (asr > -100.0) bvn = a * exp(asr) * (1.0 - c * (bs - as) * (1.0 - d * bs) / 3.0 + c * d * as * as);
            if (hk > -100.0) {
                const double b = sqrt(bs), sp = 2.5066282746310002 * phid(-b / a);
                bvn = bvn - exp(-hk / 2.0) * sp * b * (1.0 - c * bs * (1.0 - d * bs) / 3.0);
            }
            const double ah = a / 2.0;
            double sum = 0.0;
            for (int j = 0; j < 2 * ng; j++) {
                const double xs = q[FXR_N1 + j];
                asr = -(bs / xs + hk) / 2.0;
                if (asr > -100.0) {
                    const double sp = 1.0 + c * xs * (1.0 + 5.0 * d * xs), rs = q[FXR_N2 + j];
                    const double ep = exp(-(hk / 2.0) * xs / ((1.0 + rs) * (1.0 + rs))) / rs;
                    sum += exp(asr) * (sp - ep) * weight(ng, j < ng ? j : j - ng);
                }
            }
            bvn = (ah * sum - bvn) / tp;
        }
        if (r > 0.0) bvn = bvn + phid(-fmax(h, k));
        else if (h >= k) bvn = -bvn;
        else {
            const double L = h < 0.0 ? phid(k) - phid(h) : phid(-h) - phid(-k);
            bvn = L - bvn;
        }
    }
    return fmax(0.0, fmin(1.0, bvn));
}

// impact-area coefficient of an (unwrapped) angle: the bins of logistic_regression_{a,}symmetrical.py
__device__ __forceinline__ double angle_coef(const FxRiskParams &p, double a) {
    if (p.n_edges == 0) return 0.0;
    if (-p.edges[0] < a && a < p.edges[0]) return 0.0;
#pragma unroll   // constant indices into the kernel-argument block: no private copy of FxRiskParams
    for (int j = 1; j < FX_RISK_MAX_EDGES; j++) {
        if (j >= p.n_edges) break;
        if (p.edges[j - 1] <= a && a < p.edges[j]) return p.coef_pos[j];
        if (-p.edges[j - 1] >= a && a > -p.edges[j]) return p.coef_neg[j];
    }
    return p.coef_else;
}

__device__ __forceinline__ double ref_speed(double dv, double ref, double ex) { return dv < ref ? pow(dv / ref, ex) : 1.0; }

// probability of step i (ego point i) against the record q; (x, y, th) of ego point i
__device__ __forceinline__ double step_probability(const FxRiskParams &p, const double *__restrict__ q, double x, double y, double th) {
    if (q[FXR_VALID] == 0.0) return 0.0;
    if (p.prob_mode == FX_RISK_PROB_MAHALANOBIS) {
        const double d0 = x - q[FXR_M0X], d1 = y - q[FXR_M0X + 1];
        const double r0 = d0 * q[FXR_IV] + d1 * q[FXR_IV + 2], r1 = d0 * q[FXR_IV + 1] + d1 * q[FXR_IV + 3];
        const double m = r0 * d0 + r1 * d1;
        return 1.0 / (m * m);
    }
    double dmin = INFINITY;
#pragma unroll
    for (int u = 0; u < 3; u++) {
        const double dx = q[FXR_M0X + 2 * u] - x, dy = q[FXR_M0X + 2 * u + 1] - y;
        dmin = fmin(dmin, sqrt(dx * dx + dy * dy));
    }
    if (dmin > 5.0) return 0.0;
    // three axis-aligned rectangles of half extents (l/6, w/2) centred at c, c +- (l/2)(2/3)(cos th, sin th)
    const double rx = (p.ego_length / 2.0) * (2.0 / 3.0), ox = p.ego_length / 6.0, oy = p.ego_width / 2.0;
    const double ex = rx * cos(th), ey = rx * sin(th);
    const double cx[3] = {x, x + ex, x - ex}, cy[3] = {y, y + ey, y - ey};
    const double sx = q[FXR_SX], sy = q[FXR_SY];
    double prob = 0.0;
    for (int u = 0; u < 3; u++) {
        const double mx = q[FXR_M0X + 2 * u], my = q[FXR_M0X + 2 * u + 1];
        for (int c = 0; c < 3; c++) {
            const double a1 = ((cx[c] - ox) - mx) / sx, a2 = ((cy[c] - oy) - my) / sy;
            const double b1 = ((cx[c] + ox) - mx) / sx, b2 = ((cy[c] + oy) - my) / sy;
            prob += ((bvnu(a1, a2, q) - bvnu(b1, a2, q)) - bvnu(a1, b2, q)) + bvnu(b1, b2, q);
        }
    }
    return prob / 3.0;
}

// harm of ego point (x, y, th, v) against a prediction (px, py, yo, vob) of an obstacle (harm_estimation.py:282-300): the ego's
// and the obstacle's
__device__ __forceinline__ void step_harm(const FxRiskParams &p, bool prot, double f_ego, double f_obs, double x, double y, double th,
                                          double v, double yo, double vob, double px, double py, double &he, double &ho) {
    const double pdof = (yo - th) + 3.141592653589793;
    const double rel = atan2(py - y, px - x);
    const double dv = sqrt((v * v + vob * vob) + ((2.0 * v) * vob) * cos(pdof));
    const double dve = f_ego * dv, dvo = f_obs * dv;
    if (prot) {
        if (p.prot_model == FX_RISK_HARM_LOGISTIC) {
            const double ae = angle_coef(p, rel - th), ao = angle_coef(p, (3.141592653589793 + rel) - yo);
            he = 1.0 / (1.0 + exp(((-p.prot_c) - p.prot_s * dve) - ae));
            ho = 1.0 / (1.0 + exp(((-p.prot_c) - p.prot_s * dvo) - ao));
        } else {
            he = ref_speed(dve, p.prot_ref, p.prot_exp);
            ho = ref_speed(dvo, p.prot_ref, p.prot_exp);
        }
    } else {
        he = p.unprot_ego_model == FX_RISK_HARM_LOGISTIC ? 1.0 / (1.0 + exp((-p.uego_c) - p.uego_s * dve))
                                                         : ref_speed(dve, p.uego_ref, p.uego_exp);
        ho = 1.0 / (1.0 + exp(p.ped_c - p.ped_s * dvo));
    }
}

// the values of a chunk's partials (NV = 2: the first two)
enum { P_EMAX = 0, P_OMAX = 1, P_HEMAX = 2, P_HOMAX = 3, P_PMAX = 4, P_HOAT = 5, P_PNAN = 6 };

// a candidate of the batch that the pass evaluates: listed, or -- every candidate -- with all of it.need in its flags
__device__ __forceinline__ bool selected(const RiskWalkArgs &w, const RiskItemArgs &it, int64_t c) {
    return w.ids || (w.flags[c] & it.need) == it.need;
}

// One wave per (tile, chunk, obstacle): lanes = candidates j0 + 64 tile + lane of the batch [j0, j0 + nb), steps t = chunk cs ...
// of obstacle blockIdx.z.  DETAIL = false: the maxima over the chunk of harm x probability, the harm evaluated only where the
// probability is not zero.  DETAIL = true: the harm at every t < pl (risk_costs.py:109-112 take the maxima of
// the whole harm lists), and the further partials of what calc_risk returns per obstacle.  The products and their order are the same
// in both.
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

// One lane per candidate of the batch: per obstacle the chunks in chunk order, then out_ego / out_obst [n] = the maximum over the
// obstacles (0.0 without one, NaN where the candidate is not selected).  DETAIL adds col [4][K][n] = ego_risk_max | obst_risk_max |
// ego_harm_max | obst_harm_max, obstacle-major, so that the 64 lanes of a wave store 512 contiguous bytes per column, and
// obst_harm_occ [n].  (The detail entry point refuses an obstacle with pl <= 0: np.max of an empty list upstream.)
template <bool DETAIL>
__device__ __forceinline__ void items_finish_body(const RiskWalkArgs &w, const RiskItemArgs &it, const int64_t j0, const int64_t jj,
                                                  double *__restrict__ out_ego, double *__restrict__ out_obst,
                                                  double *__restrict__ col, double *__restrict__ out_occ) {
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
template <bool DETAIL>
__global__ __launch_bounds__(256) void fx_risk_items_finish_kernel(const RiskWalkArgs w, const RiskItemArgs it, const int64_t j0,
                                                                  double *__restrict__ out_ego, double *__restrict__ out_obst,
                                                                  double *__restrict__ col, double *__restrict__ out_occ) {
    items_finish_body<DETAIL>(w, it, j0, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, out_ego, out_obst, col, out_occ);
}

// Risk-cost principles (risk_costs.py:124-251) over the columns of the detail pass: one lane per listed candidate streams the K
// obstacles and accumulates as it goes -- no per-lane array, nothing in scratch.  Every lane walks the reach-set parts in the
// same order, so the part tables and the vertices are wave-uniform loads; the crossing test has no branch.
// out [7][n] = bayes | equality | maximin | ego | responsibility | total | boundary_harm (NaN where the candidate is not selected)
// every: ids == null evaluates every row, as the identity list would (the batched responsibility pass)
__device__ __forceinline__ void cost_body(const RiskCostArgs &a, const int64_t j, const bool every) {
    if (j >= a.n) return;
    const size_t n = (size_t)a.n;
    const int64_t c = a.ids ? a.ids[j] : j;
    const uint32_t fl = a.flags[c];
    const uint32_t need = FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED;
    double *__restrict__ out = a.out + j;
    if (!every && !a.ids && (fl & need) != need) {
#pragma unroll
        for (int q = 0; q < 7; q++) out[q * n] = NAN;
        return;
    }
    const int K = a.K, S = a.S;
    const int64_t ld = a.ld;
    // boundary harm: the caller's, or planner.py:369-375 on the first step outside the road
    double bh = 0.0;
    if (a.bh_in) {
        bh = a.bh_in[j];
    } else if (a.bstep && (fl & FX_FLAG_BOUNDARY)) {
        const int st = a.bstep[c];
        if (st >= 0 && st < S) bh = 1.0 / (1.0 + exp((-a.bh_c) - a.bh_s * a.planes[(3 * (size_t)S + st) * ld + c]));
    }
    const double *__restrict__ ce = a.col + j;
    double se = 0.0, so = 0.0, sabs = 0.0, mx = bh, resp = 0.0;
    for (int k = 0; k < K; k++) {
        const double er = ce[((size_t)0 * K + k) * n], orr = ce[((size_t)1 * K + k) * n];
        const double eh = ce[((size_t)2 * K + k) * n], oh = ce[((size_t)3 * K + k) * n];
        se += er;
        so += orr;
        sabs += fabs(er - orr);
        // get_maximin_costs: the harm is KEPT where the risk is below eps (upstream's gate, transcribed)
        mx = fmax(mx, fmax(eh * (er < a.eps ? 1.0 : 0.0), oh * (orr < a.eps ? 1.0 : 0.0)));
        if (a.resp_mode == FX_RISK_RESP_ACTION_SPACE) resp = resp - a.resp[k] * orr;
    }
    if (a.resp_mode == FX_RISK_RESP_REACH_SET) {
        const double *X = a.planes + c, *Y = a.planes + (size_t)S * ld + c;
        for (int e = 0; e < a.n_entries; e++) {
            unsigned inside = 0u;
            for (int pt = a.entry_off[e]; pt < a.entry_off[e + 1]; pt++) {
                const int st = a.part_step[pt], v0 = a.vert_off[pt], v1 = a.vert_off[pt + 1];
                if (v1 <= v0) continue;
                const double px = X[(size_t)st * ld], py = Y[(size_t)st * ld];
                double xj = a.verts[2 * (size_t)(v1 - 1)], yj = a.verts[2 * (size_t)(v1 - 1) + 1];
                unsigned par = 0u;
                for (int v = v0; v < v1; v++) {   // even-odd crossings of the ray towards +x; a horizontal edge never straddles
                    const double xi = a.verts[2 * (size_t)v], yi = a.verts[2 * (size_t)v + 1];
                    par ^= (unsigned)((yi > py) != (yj > py)) & (unsigned)(px < (xj - xi) * (py - yi) / (yj - yi) + xi);
                    xj = xi;
                    yj = yi;
                }
                inside |= par;
            }
            const double r = ce[((size_t)1 * K + a.entry_obs[e]) * n];
            resp = inside ? resp : resp - r;
        }
    }
    double bayes = 0.0, equal = 0.0, maximin = 0.0, ego = 0.0;
    if (K > 0) {
        bayes = ((se + so) + bh) / (double)(2 * K);
        equal = sabs / (double)K;
        maximin = pow(mx, a.scale);
        ego = se + bh;
    } else {
        resp = 0.0;
    }
    out[0 * n] = bayes;
    out[1 * n] = equal;
    out[2 * n] = maximin;
    out[3 * n] = ego;
    out[4 * n] = resp;
    out[5 * n] = (((a.w[0] * bayes + a.w[1] * equal) + a.w[2] * maximin) + a.w[3] * ego) + a.w[4] * resp;
    out[6 * n] = bh;
}
__global__ __launch_bounds__(256) void fx_risk_cost_kernel(const RiskCostArgs a) {
    cost_body(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, false);
}

// The responsibility cost as one more weighted term of the step's cost sum: one lane per listed candidate re-sums the step's raw
// cost rows (FX_MODE_WRITE_COSTMAP) with w_resp * resp inserted in front of entry a.at -- its place in the name-sorted list,
// between `prediction` and `velocity_offset` -- in the order and with the operations of fx_predprob_finish_kernel: sum = -0.0;
// sum += w * c per term; a deferred step (fx_obstacle_kernel.h) added the terms behind the prediction as ONE addend, which the new
// term then joins.  The prediction entry is the step's own, or a.pred [n] (the prob of a collision-probability pass over the same
// candidates).  resp [n] is row 4 of fx_risk_cost_kernel's output.
__device__ __forceinline__ void resp_sum_body(const RespSumArgs &a, const int64_t j) {
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
__global__ __launch_bounds__(256) void fx_resp_finish_kernel(const RespSumArgs a) {
    resp_sum_body(a, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// arg-min over the n entries of ego + obst (SUM) or of val = ego alone, NaN = not selected or not comparable, ties to the lower
// candidate index, -1 when nothing is left: ONE workgroup of 1024 lanes, the lexicographic (cost, index) reduction of fx_select.h
template <bool SUM>
__device__ __forceinline__ void risk_argmin(const double *__restrict__ ego, const double *__restrict__ obst, int64_t n,
                                            const int64_t *__restrict__ ids, long long *__restrict__ out) {
    double bc;
    long long bi;
    fx_lex_block_min(n, ids, [=](int64_t j, long long, double &s) {
        const double e = ego[j], o = SUM ? obst[j] : 0.0;
        s = SUM ? e + o : e;
        return e == e && o == o;
    }, bc, bi);
    if (threadIdx.x == 0) out[0] = bi == FX_LEX_NONE ? -1LL : bi;
}

__global__ __launch_bounds__(1024) void fx_risk_argmin_kernel(const double *__restrict__ ego, const double *__restrict__ obst, int64_t n,
                                                              const int64_t *__restrict__ ids, long long *__restrict__ out) {
    risk_argmin<true>(ego, obst, n, ids, out);
}

// the same over the total of the risk-cost pass
__global__ __launch_bounds__(1024) void fx_risk_cost_argmin_kernel(const double *__restrict__ val, int64_t n, const int64_t *__restrict__ ids,
                                                                   long long *__restrict__ out) {
    risk_argmin<false>(val, nullptr, n, ids, out);
}

// ---- the responsibility pass of several agents in one call (fx_eval_responsibility_cost_batch) ----
// The row of flat index `at` (an item of the item launch, a workgroup of the other launches) among n_rows rows whose first indices
// `first0` ascend: the last row that starts at or before `at` (fx_predprob_kernel.h row_of).  A row without
// an item shares its first index with the row behind it, which is the one found.  One load per 64 rows and a ballot: `at` is
// wave-uniform, so is the answer.
template <typename T>
__device__ __forceinline__ int batch_row_of(const T *__restrict__ first0, const int n_rows, const int64_t at) {
    const int lane = threadIdx.x & 63;
    int r = 0;
    for (int b = 0; b < n_rows; b += 64) r += __popcll(__ballot(b + lane < n_rows && (int64_t)first0[b + lane] <= at));
    return __builtin_amdgcn_readfirstlane(r - 1);
}

// One wave per item of a round: grid.x = the round's items exactly.  rows, item0: of the round.  Tile, chunk and obstacle of the
// item come from blockIdx alone, so the row's fields, the record and FxRiskParams are scalar loads; from there on the loop of
// fx_risk_item_kernel<true> with ids == null in its own text (that kernel is to stay what it is), the same seven partials in the
// same layout [K][chunks][7][nb] of the row's segment.
__global__ __launch_bounds__(64) void fx_risk_batch_item_kernel(const RiskBatchRow *__restrict__ rows, const int64_t *__restrict__ item0,
                                                                const int n_rows) {
    const int64_t at = blockIdx.x;
    const RiskBatchRow &r = rows[batch_row_of(item0, n_rows, at)];
    const RiskWalkArgs &w = r.w;
    const RiskItemArgs &it = r.it;
    const FxRiskParams &p = *it.params;
    const int64_t local = at - r.item0, tiles = it.nb / 64, rest = local / tiles;
    const int lane = threadIdx.x, S = w.S;
    const int k = (int)(rest / it.chunks), ch = (int)(rest % it.chunks);
    const double *__restrict__ o = w.obs + (size_t)k * FXO_STRIDE;
    const int pl = min(S - 1, (int)o[FXO_NPOS]);
    const int t_a = ch * it.cs, t_b = min(pl, t_a + it.cs);
    if (t_a >= t_b) return;   // (wave-uniform)
    const int64_t jj = (local % tiles) * 64 + lane;
    if (jj >= r.count) return;   // (count <= nb, first + count <= n)
    const int64_t c = r.first + jj;
    if ((w.flags[c] & it.need) != it.need) return;   // (NaN rows from the finish kernel)
    const int64_t ld = w.ld;
    const double *__restrict__ X = w.planes + c, *__restrict__ Y = X + (size_t)S * ld, *__restrict__ TH = Y + (size_t)S * ld,
                 *__restrict__ V = TH + (size_t)S * ld;
    const bool prot = o[FXO_CLS] == (double)FX_RISK_CLASS_PROTECTED;
    const double me = p.ego_mass, mo = o[FXO_MASS];
    const double f_ego = mo / (me + mo), f_obs = me / (me + mo);
    double e_max = -INFINITY, o_max = -INFINITY, he_max = -INFINITY, ho_max = -INFINITY, p_max = -INFINITY, ho_at = 0.0;
    bool p_nan = false;
    for (int t = t_a; t < t_b; t++) {
        const int i = t + 1;
        const double *__restrict__ q = w.rec + ((size_t)k * S + i) * FXR_STRIDE;
        const double prob = fxrisk::step_probability(p, q, X[(size_t)i * ld], Y[(size_t)i * ld], TH[(size_t)i * ld]);
        const size_t kt = (size_t)k * w.P + t;
        double he, ho;
        fxrisk::step_harm(p, prot, f_ego, f_obs, X[(size_t)t * ld], Y[(size_t)t * ld], TH[(size_t)t * ld], V[(size_t)t * ld], w.yaw[kt],
                          w.vo[kt], w.pos[2 * kt], w.pos[2 * kt + 1], he, ho);
        const double re = prob != 0.0 ? he * prob : 0.0;
        const double ro = prob != 0.0 ? ho * prob : 0.0;
        he_max = fmax(he_max, he);
        ho_max = fmax(ho_max, ho);
        p_nan = p_nan || prob != prob;
        if (prob > p_max) { p_max = prob; ho_at = ho; }
        e_max = fmax(e_max, re);
        o_max = fmax(o_max, ro);
    }
    const size_t nb = (size_t)it.nb;
    double *__restrict__ out = it.part + (((size_t)k * it.chunks + ch) * 7) * nb + jj;
    out[(size_t)P_EMAX * nb] = e_max;
    out[(size_t)P_OMAX * nb] = o_max;
    out[(size_t)P_HEMAX * nb] = he_max;
    out[(size_t)P_HOMAX * nb] = ho_max;
    out[(size_t)P_PMAX * nb] = p_max;
    out[(size_t)P_HOAT * nb] = ho_at;
    out[(size_t)P_PNAN * nb] = p_nan ? 1.0 : 0.0;
}

// One lane per (row, candidate) of a round: grid.x = the rows' workgroups of 256; the chunk combination of
// fx_risk_items_finish_kernel<true> (the same function) into the agent's columns
__global__ __launch_bounds__(256) void fx_risk_batch_finish_kernel(const RiskBatchRow *__restrict__ rows, const int32_t *__restrict__ fin0,
                                                                   const int n_rows) {
    const RiskBatchRow &r = rows[batch_row_of(fin0, n_rows, (int64_t)blockIdx.x)];
    const int64_t jj = (int64_t)(blockIdx.x - r.fin0) * blockDim.x + threadIdx.x;
    if (jj < r.count) items_finish_body<true>(r.w, r.it, r.first, jj, r.ego, r.obst, r.col, r.occ);
}

// Behind the last round, one launch each over all listed agents: one lane per (agent, candidate), the agent of a workgroup found
// through blk0[]; the cost kernel's and the re-sum's own functions on the agent's argument block
__global__ __launch_bounds__(256) void fx_risk_batch_cost_kernel(const RiskCostArgs *__restrict__ cost, const int32_t *__restrict__ blk0,
                                                                 const int n_agents) {
    const int a = batch_row_of(blk0, n_agents, (int64_t)blockIdx.x);
    cost_body(cost[a], (int64_t)(blockIdx.x - blk0[a]) * blockDim.x + threadIdx.x, true);
}
__global__ __launch_bounds__(256) void fx_risk_batch_sum_kernel(const RespSumArgs *__restrict__ sum, const int32_t *__restrict__ blk0,
                                                                const int n_agents) {
    const int a = batch_row_of(blk0, n_agents, (int64_t)blockIdx.x);
    resp_sum_body(sum[a], (int64_t)(blockIdx.x - blk0[a]) * blockDim.x + threadIdx.x);
}

// One workgroup of 1024 lanes per listed agent, the predicate of fx_predprob_argmin_kernel over the agent's total: selectable,
// neither colliding nor off the road, NaN skipped; out[2 agent] = index (-1: none), out[2 agent + 1] = the cost's bits
__global__ __launch_bounds__(1024) void fx_risk_batch_argmin_kernel(const RespSumArgs *__restrict__ sum, long long *__restrict__ out) {
    const RespSumArgs &a = sum[blockIdx.x];
    const double *__restrict__ total = a.total;
    const uint32_t *__restrict__ flags = a.flags;
    double bc;
    long long bi;
    fx_lex_block_min(a.n, nullptr, [=](int64_t j, long long c, double &t) {
        const uint32_t f = flags[c];
        t = total[j];
        return (f & FX_FLAG_SELECTABLE) && !(f & (FX_FLAG_COLLISION | FX_FLAG_BOUNDARY)) && t == t;
    }, bc, bi);
    if (threadIdx.x == 0) {
        const bool none = bi == FX_LEX_NONE;
        out[2 * blockIdx.x] = none ? -1LL : bi;
        out[2 * blockIdx.x + 1] = __double_as_longlong(none ? (double)NAN : bc);
    }
}

// ---- the plain risk pass of several agents in one call, with or without id lists (fx_eval_risk_batch) ----
// One wave per item of a round, as fx_risk_batch_item_kernel finds it; lane jj of a row handles list position first + jj: the
// candidate ids[first + jj] of a row with a list -- evaluated whatever its flags, as selected() has it -- or candidate first + jj,
// which then needs all of it.need.  The choice is the row's, so wave-uniform.  From there on the loop of fx_risk_item_kernel<false>
// in its own text (that kernel is to stay what it is): the harm only where the probability is not zero, the two partials in the
// layout [K][chunks][2][nb] of the row's segment.  FxRiskParams through the row's pointer, never by value.
__global__ __launch_bounds__(64) void fx_risk_list_batch_item_kernel(const RiskBatchRow *__restrict__ rows, const int64_t *__restrict__ item0,
                                                                     const int n_rows) {
    const int64_t at = blockIdx.x;
    const RiskBatchRow &r = rows[batch_row_of(item0, n_rows, at)];
    const RiskWalkArgs &w = r.w;
    const RiskItemArgs &it = r.it;
    const FxRiskParams &p = *it.params;
    const int64_t local = at - r.item0, tiles = it.nb / 64, rest = local / tiles;
    const int lane = threadIdx.x, S = w.S;
    const int k = (int)(rest / it.chunks), ch = (int)(rest % it.chunks);
    const double *__restrict__ o = w.obs + (size_t)k * FXO_STRIDE;
    const int pl = min(S - 1, (int)o[FXO_NPOS]);
    const int t_a = ch * it.cs, t_b = min(pl, t_a + it.cs);
    if (t_a >= t_b) return;   // (wave-uniform)
    const int64_t jj = (local % tiles) * 64 + lane;
    if (jj >= r.count) return;   // (count <= nb, first + count <= n)
    const int64_t c = w.ids ? w.ids[r.first + jj] : r.first + jj;
    if (!selected(w, it, c)) return;   // (NaN rows from the finish kernel)
    const int64_t ld = w.ld;
    const double *__restrict__ X = w.planes + c, *__restrict__ Y = X + (size_t)S * ld, *__restrict__ TH = Y + (size_t)S * ld,
                 *__restrict__ V = TH + (size_t)S * ld;
    const bool prot = o[FXO_CLS] == (double)FX_RISK_CLASS_PROTECTED;
    const double me = p.ego_mass, mo = o[FXO_MASS];
    const double f_ego = mo / (me + mo), f_obs = me / (me + mo);
    double e_max = -INFINITY, o_max = -INFINITY;
    for (int t = t_a; t < t_b; t++) {
        const int i = t + 1;
        const double *__restrict__ q = w.rec + ((size_t)k * S + i) * FXR_STRIDE;
        const double prob = fxrisk::step_probability(p, q, X[(size_t)i * ld], Y[(size_t)i * ld], TH[(size_t)i * ld]);
        double re = 0.0, ro = 0.0;
        if (prob != 0.0) {
            const size_t kt = (size_t)k * w.P + t;
            double he, ho;
            fxrisk::step_harm(p, prot, f_ego, f_obs, X[(size_t)t * ld], Y[(size_t)t * ld], TH[(size_t)t * ld], V[(size_t)t * ld], w.yaw[kt],
                              w.vo[kt], w.pos[2 * kt], w.pos[2 * kt + 1], he, ho);
            re = he * prob;
            ro = ho * prob;
        }
        e_max = fmax(e_max, re);
        o_max = fmax(o_max, ro);
    }
    const size_t nb = (size_t)it.nb;
    double *__restrict__ out = it.part + (((size_t)k * it.chunks + ch) * 2) * nb + jj;
    out[(size_t)P_EMAX * nb] = e_max;
    out[(size_t)P_OMAX * nb] = o_max;
}

// One lane per (row, list position) of a round: the chunk combination of fx_risk_items_finish_kernel<false> (the same function)
// into the agent's rows of the call's concatenated outputs
__global__ __launch_bounds__(256) void fx_risk_list_batch_finish_kernel(const RiskBatchRow *__restrict__ rows, const int32_t *__restrict__ fin0,
                                                                        const int n_rows) {
    const RiskBatchRow &r = rows[batch_row_of(fin0, n_rows, (int64_t)blockIdx.x)];
    const int64_t jj = (int64_t)(blockIdx.x - r.fin0) * blockDim.x + threadIdx.x;
    if (jj < r.count) items_finish_body<false>(r.w, r.it, r.first, jj, r.ego, r.obst, nullptr, nullptr);
}

// One workgroup of 1024 lanes per listed agent: fx_risk_argmin_kernel's reduction over the agent's rows -- the candidate INDEX of
// the minimum of ego + obst, ties to the lower candidate index whatever the list's order, -1 when nothing is left (or the agent
// has no row: agent_row < 0)
__global__ __launch_bounds__(1024) void fx_risk_list_batch_argmin_kernel(const RiskBatchRow *__restrict__ rows, const int32_t *__restrict__ agent_row,
                                                                         long long *__restrict__ out) {
    const int row = agent_row[blockIdx.x];
    if (row < 0) {   // (uniform over the workgroup)
        if (threadIdx.x == 0) out[blockIdx.x] = -1LL;
        return;
    }
    const RiskBatchRow &r = rows[row];
    risk_argmin<true>(r.ego, r.obst, r.w.n, r.w.ids, out + blockIdx.x);
}

// ---- the detail and cost passes of several agents in one call, with or without id lists (fx_eval_risk_costs_batch; DESIGN.md
// section 21) ----
// One wave per item of a round, as fx_risk_batch_item_kernel finds it; lane jj of a row handles list position first + jj: the
// candidate ids[first + jj] of a row with a list -- evaluated whatever its flags, as selected() has it -- or candidate first + jj,
// which then needs all of it.need.  The choice is the row's, so wave-uniform, and the index load stands in front of the walk: once
// the four plane pointers are formed neither the list pointer nor the index is live in the loop.  From there on the loop of
// fx_risk_item_kernel<true> in its own text (that kernel is to stay what it is): the harm at every t < pl, the seven partials in
// the layout [K][chunks][7][nb] of the row's segment.  FxRiskParams through the row's pointer, never by value.
__global__ __launch_bounds__(64) void fx_risk_costs_batch_item_kernel(const RiskBatchRow *__restrict__ rows, const int64_t *__restrict__ item0,
                                                                      const int n_rows) {
    const int64_t at = blockIdx.x;
    const RiskBatchRow &r = rows[batch_row_of(item0, n_rows, at)];
    const RiskWalkArgs &w = r.w;
    const RiskItemArgs &it = r.it;
    const FxRiskParams &p = *it.params;
    const int64_t local = at - r.item0, tiles = it.nb / 64, rest = local / tiles;
    const int lane = threadIdx.x, S = w.S;
    const int k = (int)(rest / it.chunks), ch = (int)(rest % it.chunks);
    const double *__restrict__ o = w.obs + (size_t)k * FXO_STRIDE;
    const int pl = min(S - 1, (int)o[FXO_NPOS]);
    const int t_a = ch * it.cs, t_b = min(pl, t_a + it.cs);
    if (t_a >= t_b) return;   // (wave-uniform)
    const int64_t jj = (local % tiles) * 64 + lane;
    if (jj >= r.count) return;   // (count <= nb, first + count <= n)
    const int64_t c = w.ids ? w.ids[r.first + jj] : r.first + jj;
    if (!selected(w, it, c)) return;   // (NaN rows from the finish kernel)
    const int64_t ld = w.ld;
    const double *__restrict__ X = w.planes + c, *__restrict__ Y = X + (size_t)S * ld, *__restrict__ TH = Y + (size_t)S * ld,
                 *__restrict__ V = TH + (size_t)S * ld;
    const bool prot = o[FXO_CLS] == (double)FX_RISK_CLASS_PROTECTED;
    const double me = p.ego_mass, mo = o[FXO_MASS];
    const double f_ego = mo / (me + mo), f_obs = me / (me + mo);
    double e_max = -INFINITY, o_max = -INFINITY, he_max = -INFINITY, ho_max = -INFINITY, p_max = -INFINITY, ho_at = 0.0;
    bool p_nan = false;
    for (int t = t_a; t < t_b; t++) {
        const int i = t + 1;
        const double *__restrict__ q = w.rec + ((size_t)k * S + i) * FXR_STRIDE;
        const double prob = fxrisk::step_probability(p, q, X[(size_t)i * ld], Y[(size_t)i * ld], TH[(size_t)i * ld]);
        const size_t kt = (size_t)k * w.P + t;
        double he, ho;
        fxrisk::step_harm(p, prot, f_ego, f_obs, X[(size_t)t * ld], Y[(size_t)t * ld], TH[(size_t)t * ld], V[(size_t)t * ld], w.yaw[kt],
                          w.vo[kt], w.pos[2 * kt], w.pos[2 * kt + 1], he, ho);
        const double re = prob != 0.0 ? he * prob : 0.0;
        const double ro = prob != 0.0 ? ho * prob : 0.0;
        he_max = fmax(he_max, he);
        ho_max = fmax(ho_max, ho);
        p_nan = p_nan || prob != prob;
        if (prob > p_max) { p_max = prob; ho_at = ho; }
        e_max = fmax(e_max, re);
        o_max = fmax(o_max, ro);
    }
    const size_t nb = (size_t)it.nb;
    double *__restrict__ out = it.part + (((size_t)k * it.chunks + ch) * 7) * nb + jj;
    out[(size_t)P_EMAX * nb] = e_max;
    out[(size_t)P_OMAX * nb] = o_max;
    out[(size_t)P_HEMAX * nb] = he_max;
    out[(size_t)P_HOMAX * nb] = ho_max;
    out[(size_t)P_PMAX * nb] = p_max;
    out[(size_t)P_HOAT * nb] = ho_at;
    out[(size_t)P_PNAN * nb] = p_nan ? 1.0 : 0.0;
}

// (The finish launch of a round is fx_risk_batch_finish_kernel as it stands: items_finish_body<true> reads the row's list through
// w.ids.  The risk arg-min is fx_risk_list_batch_argmin_kernel as it stands.)

// Behind the last round, one launch over the agents WITH cost parameters (cost [n_cost], compact, in call order): one lane per
// (agent, list position), the agent of a workgroup found through blk0[]; the cost kernel's own function with the per-agent call's
// rule for an agent without a list (every = false: NaN rows where a flag of VALID, FEASIBLE, RETURNED is missing)
__global__ __launch_bounds__(256) void fx_risk_costs_batch_cost_kernel(const RiskCostArgs *__restrict__ cost, const int32_t *__restrict__ blk0,
                                                                       const int n_cost) {
    const int a = batch_row_of(blk0, n_cost, (int64_t)blockIdx.x);
    cost_body(cost[a], (int64_t)(blockIdx.x - blk0[a]) * blockDim.x + threadIdx.x, false);
}

// One workgroup of 1024 lanes per agent with cost parameters: fx_risk_cost_argmin_kernel's reduction over the agent's totals -- the
// candidate INDEX of the minimum, ties to the lower candidate index whatever the list's order, NaN skipped, -1 when nothing is left
__global__ __launch_bounds__(1024) void fx_risk_costs_batch_argmin_kernel(const RiskCostArgs *__restrict__ cost, long long *__restrict__ out) {
    const RiskCostArgs &a = cost[blockIdx.x];
    risk_argmin<false>(a.out + 5 * (size_t)a.n, nullptr, a.n, a.ids, out + blockIdx.x);
}

// Behind them, where the caller asked for a column: the agents' column planes into the call's concatenated columns, which then
// come down in one copy each.  One workgroup per 1 024 doubles of a segment, the segment found through blk0[]
__global__ __launch_bounds__(256) void fx_risk_costs_batch_gather_kernel(const RiskCopySeg *__restrict__ seg, const int32_t *__restrict__ blk0,
                                                                         const int n_seg) {
    const int s = batch_row_of(blk0, n_seg, (int64_t)blockIdx.x);
    const RiskCopySeg &g = seg[s];
    const int64_t j0 = (int64_t)(blockIdx.x - blk0[s]) * 1024 + threadIdx.x;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t j = j0 + 256 * u;
        if (j < g.n) g.dst[j] = g.src[j];
    }
}

}  // namespace fxrisk
