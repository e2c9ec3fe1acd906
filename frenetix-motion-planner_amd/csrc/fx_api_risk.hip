// fx_api_risk.hip -- C-ABI of the trajectory risk (fx_risk_kernel.h): the obstacle tables of an agent and
// the risk pass with its arg-min over the materialised bundle of the last plan step (or, for listed candidates of a step that stored
// none, over the agent's sparse set: fx_api_materialise.hip); the reach sets of an agent and the detail /
// risk-cost pass.  The two evaluations share one host path (RiskPass) and one device block.  Nothing of
// this runs in a plan step.  The collision probability as the prediction cost (fx_predprob_kernel.h) is a third
// entrance on the same host path: the same checks, records, uploads and block; fx_eval_prediction_prob_batch
// is that pass for several agents in one call: the same checks and records per agent, one staging buffer each for records and tables;
// fx_eval_responsibility_cost_batch is the responsibility pass for several agents in one call, and
// fx_eval_risk_batch the plain risk pass for several agents, each with an id list or none, and
// fx_eval_risk_costs_batch the detail and cost passes for several agents, with lists and cost parameters each.
#include <atomic>
#include <cmath>
#include <memory>
#include <vector>

#include "fx_pass.h"
#include "fx_risk_args.h"

extern "C" hipError_t fx_launch_risk(const RiskWalkArgs *walk, const RiskItemArgs *items, double *out_ego, double *out_obst, double *col,
                                     double *out_occ, const RiskCostArgs *cost, long long *out_idx, hipEvent_t ev_start,
                                     hipEvent_t ev_stop, hipStream_t stream, const RespSumArgs *resp, long long *resp_idx);
extern "C" hipError_t fx_launch_predprob(const PredProbArgs *args, long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                                         hipStream_t stream);
// (weak, like the chunk rule below: a host-only program that links these files against launcher stubs of its own need not define
// the launchers that came after it was written; fx_eval_prediction_prob_batch reports their absence)
extern "C" __attribute__((weak)) hipError_t fx_launch_predprob_batch(const PredProbBatchArgs *t, const PredProbRound *rounds, int n_rounds,
                                                                     long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                                                                     hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t fx_launch_risk_batch(const RiskBatchArgs *t, const RiskBatchRound *rounds, int n_rounds,
                                                                 long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                                                                 hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t fx_launch_risk_list_batch(const RiskListBatchArgs *t, const RiskBatchRound *rounds, int n_rounds,
                                                                      long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                                                                      hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t fx_launch_risk_costs_batch(const RiskCostBatchArgs *t, const RiskBatchRound *rounds, int n_rounds,
                                                                       long long *out_idx, long long *cost_idx, hipEvent_t ev_start,
                                                                       hipEvent_t ev_stop, hipStream_t stream);
extern "C" __attribute__((weak)) int32_t fx_predprob_chunk_steps(int64_t n, int32_t S, int32_t K);   // (fx_kernels.hip: the rule, or what a test forces)

namespace {
// Gauss-Legendre nodes on [-1, 1], positive half: 6, 12 and 20 points (Genz 2004)
const double kX6[3] = {0.9324695142031522, 0.6612093864662647, 0.2386191860831970};
const double kX12[6] = {0.9815606342467191, 0.9041172563704750, 0.7699026741943050,
                        0.5873179542866171, 0.3678314989981802, 0.1252334085114692};
const double kX20[10] = {0.9931285991850949, 0.9639719272779138, 0.9122344282513259, 0.8391169718222188, 0.7463319064601508,
                         0.6360536807265150, 0.5108670019508271, 0.3737060887154196, 0.2277858511416451, 0.07652652113349733};
}  // namespace

struct FxRiskAgent {
    int K = 0, P = 0;
    std::vector<double> pos, cov, cov_inv, yaw, v, obs;   // obs [K][FXO_STRIDE]
    std::vector<int32_t> n_pos, n_yaw, n_v;
    bool have_inv = false;
    // reach sets (fx_set_reach_sets_agent): entries index the K obstacles above, so new obstacles clear them
    std::vector<int32_t> rs_obs, rs_off, rs_step, rs_voff;
    std::vector<double> rs_verts;
};

struct FxRiskState {
    explicit FxRiskState(FxContext *c) : block(&c->dev_bytes) {}
    std::vector<FxRiskAgent> agents;
    FxDeviceBlock block;     // the block of a risk pass (RiskPass): grows to the largest call, never shrinks
    FxEventPair ev;          // around a pass's launches; read at once into the two times below
    float last_ms = 0.f;
    float last_pp_ms = -1.f;   // fx_eval_prediction_prob_agent
    int32_t last_rounds = -1;  // fx_eval_risk_costs_batch: the rounds of scratch of the last call
};

void fx_risk_release(FxRiskState *r) { delete r; }

static FxRiskState *risk_state(FxContext *c) {
    if (!c->risk) c->risk.reset(new FxRiskState(c));
    if ((int)c->risk->agents.size() < c->max_agents) c->risk->agents.resize(c->max_agents);
    return c->risk.get();
}

extern "C" int32_t fx_set_risk_obstacles_agent(FxContext *c, int32_t agent, int32_t K, int32_t P, const double *pos, const double *cov,
                                               const double *cov_inv, const double *yaw, const double *v, const int32_t *n_pos,
                                               const int32_t *n_yaw, const int32_t *n_v, const double *length, const double *width,
                                               const double *mass, const int32_t *cls) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (agent < 0 || agent >= c->max_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
    if (K < 0 || (K > 0 && (P < 1 || !pos || !cov || !yaw || !v || !n_pos || !n_yaw || !n_v || !length || !width || !mass || !cls)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "risk obstacle arrays inconsistent (K=%d, P=%d)", K, P);
    for (int k = 0; k < K; k++) {
        if (n_pos[k] < 0 || n_pos[k] > P || n_yaw[k] < 0 || n_yaw[k] > P || n_v[k] < 0 || n_v[k] > P)
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: prediction lengths (%d, %d, %d) outside [0, P=%d]", k, n_pos[k], n_yaw[k],
                           n_v[k], P);
        if (cls[k] != FX_RISK_CLASS_PROTECTED && cls[k] != FX_RISK_CLASS_UNPROTECTED)
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: class %d", k, cls[k]);
    }
    FxRiskAgent &a = risk_state(c)->agents[agent];
    a = FxRiskAgent();
    a.K = K;
    a.P = P;
    if (K == 0) return FX_OK;
    const size_t KP = (size_t)K * P;
    a.pos.assign(pos, pos + 2 * KP);
    a.cov.assign(cov, cov + 4 * KP);
    a.have_inv = cov_inv != nullptr;
    if (cov_inv) a.cov_inv.assign(cov_inv, cov_inv + 4 * KP);
    a.yaw.assign(yaw, yaw + KP);
    a.v.assign(v, v + KP);
    a.n_pos.assign(n_pos, n_pos + K);
    a.n_yaw.assign(n_yaw, n_yaw + K);
    a.n_v.assign(n_v, n_v + K);
    a.obs.assign((size_t)K * FXO_STRIDE, 0.0);
    for (int k = 0; k < K; k++) {
        double *o = a.obs.data() + (size_t)k * FXO_STRIDE;
        o[FXO_LEN] = length[k];
        o[FXO_WID] = width[k];
        o[FXO_MASS] = mass[k];
        o[FXO_CLS] = (double)cls[k];
        o[FXO_NPOS] = (double)n_pos[k];
    }
    return FX_OK;
}

// the (obstacle, ego step) records: means, standardisation, |rho| branch and node terms -- once for all candidates
static void build_records(const FxRiskAgent &a, int S, bool mahalanobis, std::vector<double> &rec) {
    rec.assign((size_t)a.K * S * FXR_STRIDE, 0.0);
    for (int k = 0; k < a.K; k++) {
        const double len = a.obs[(size_t)k * FXO_STRIDE + FXO_LEN];
        for (int i = 1; i < S; i++) {
            double *q = rec.data() + ((size_t)k * S + i) * FXR_STRIDE;
            if (i >= a.n_pos[k]) continue;   // collision_probability.py:239: the prediction ends before ego point i
            q[FXR_VALID] = 1.0;
            const size_t p0 = (size_t)k * a.P + (i - 1);
            const double mx = a.pos[2 * p0], my = a.pos[2 * p0 + 1];
            const double yw = a.yaw[(size_t)k * a.P + i];   // yaw of prediction i, mean of prediction i - 1 (:182-185)
            const double dx = std::cos(yw) * len / 2.0, dy = std::sin(yw) * len / 2.0;
            const double m[6] = {mx, my, mx + dx, my + dy, mx - dx, my - dy};
            for (int u = 0; u < 6; u++) q[FXR_M0X + u] = m[u];
            if (mahalanobis) {
                for (int u = 0; u < 4; u++) q[FXR_IV + u] = a.cov_inv[4 * p0 + u];
                continue;
            }
            double cv[4] = {a.cov[4 * p0], a.cov[4 * p0 + 1], a.cov[4 * p0 + 2], a.cov[4 * p0 + 3]};
            if (cv[0] == 0.0 && cv[1] == 0.0 && cv[2] == 0.0 && cv[3] == 0.0) { cv[0] = 0.1; cv[1] = 0.0; cv[2] = 0.0; cv[3] = 0.1; }
            const double sx = std::sqrt(cv[0]), sy = std::sqrt(cv[3]);
            const double rho = cv[2] / sy / sx;   // mvnun: covar(2,1) / stdev(2) / stdev(1)
            q[FXR_SX] = sx;
            q[FXR_SY] = sy;
            q[FXR_RHO] = rho;
            const double ar = std::fabs(rho);
            const int ng = ar < 0.3 ? 3 : (ar < 0.75 ? 6 : 10);
            const double *x = ng == 3 ? kX6 : (ng == 6 ? kX12 : kX20);
            q[FXR_NG] = ng;
            if (rho == 0.0) {
                q[FXR_BRANCH] = 0;
            } else if (ar < 0.925) {
                q[FXR_BRANCH] = 1;
                const double asr = std::asin(rho) / 2.0;
                q[FXR_ASR] = asr;
                for (int j = 0; j < ng; j++) {
                    q[FXR_N1 + j] = std::sin(asr * (1.0 - x[j]));
                    q[FXR_N1 + ng + j] = std::sin(asr * (1.0 + x[j]));
                }
            } else if (ar < 1.0) {
                q[FXR_BRANCH] = 2;
                const double as = 1.0 - rho * rho, aa = std::sqrt(as), ah = aa / 2.0;
                q[FXR_ASR] = as;
                q[FXR_A] = aa;
                for (int j = 0; j < ng; j++) {
                    const double u0 = ah * (1.0 - x[j]), u1 = ah * (1.0 + x[j]);
                    q[FXR_N1 + j] = u0 * u0;
                    q[FXR_N1 + ng + j] = u1 * u1;
                    q[FXR_N2 + j] = std::sqrt(1.0 - q[FXR_N1 + j]);
                    q[FXR_N2 + ng + j] = std::sqrt(1.0 - q[FXR_N1 + ng + j]);
                }
            } else {
                q[FXR_BRANCH] = 3;
            }
        }
    }
}

// One evaluation over candidates of an agent's last plan step, the host path of fx_eval_risk_agent and fx_eval_risk_costs_agent:
// what risk_check established and, after risk_stage, where the parts of the device block lie.
struct RiskPass {
    FxContext *c;
    FxRiskState *r;
    int32_t agent;
    const FxAgentSlot *s;   // of the agent
    const FxRiskAgent *a;
    int S, K, P;
    bool maha;
    int64_t n;             // candidates evaluated: the listed ones, or all C
    const int64_t *ids;    // the caller's list, or null
    // where the candidates' rows lie: the step's bundle, or -- a step that stored none -- the agent's sparse set
    // (fx_api_materialise.hip), addressed by `pos`, the listed candidates' positions in it
    bool sparse = false;
    FxSparseView set;
    std::vector<int64_t> pos;
    const double *planes;
    int64_t ld;
    const uint32_t *flags;
    const int32_t *bstep;
    std::vector<double> rec;
    size_t nE = 0, nP = 0, nV = 0;   // reach-set entries, parts and vertices of a cost pass in reach-set mode
    char *base;
    size_t o_rec, o_obs, o_pos, o_yaw, o_v, o_ids, o_ego, o_obst, o_idx;
    size_t o_occ, o_col;                                                 // detail pass only
    size_t o_out, o_bh, o_resp, o_eobs, o_eoff, o_pst, o_voff, o_vert;   // cost pass only
    size_t o_pstep, o_pprob, o_pobs, o_ptot, o_pbest;                    // prediction-probability pass only
    RiskItemArgs it{};       // the items of the walk (fx_risk_kernel.h): their partials at o_part, the parameters at o_prm
    size_t o_part, o_prm;
    const FxRiskParams *prm;   // the call's parameters (risk_check)
    size_t o_rresp, o_rtot, o_rpred, o_rbest;                            // responsibility pass only

    double *D(size_t o) const { return reinterpret_cast<double *>(base + o); }
    int32_t *I(size_t o) const { return reinterpret_cast<int32_t *>(base + o); }
    const int64_t *d_ids() const { return ids ? reinterpret_cast<const int64_t *>(base + o_ids) : nullptr; }
    hipError_t up(size_t o, const void *src, size_t bytes) const {
        return bytes ? hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    }
    hipError_t down(double *dst, size_t o, size_t count) const {
        return (dst && count) ? hipMemcpyAsync(dst, base + o, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    }
};

// The checks of a pass in the order the entry points report them: the plan step, FxRiskParams, the id list, the obstacle lists.
// have_out: the entry point's output pointers are there.  detail: the checks of fx_eval_risk_costs_agent -- it reports missing
// outputs with params, and refuses an obstacle that calc_risk cannot evaluate (the plain pass skips it).
static int risk_check(RiskPass &q, FxContext *c, int32_t agent, const FxRiskParams *params, int64_t n_ids, const int64_t *ids,
                      bool have_out, bool detail, bool need_v = true) {
    FX_TRY(check_agent(c, agent));
    const FxAgentSlot &s = c->slots[agent];
    q.sparse = !(s.mode & FX_MODE_WRITE_BUNDLE);
    if (q.sparse) {   // every listed candidate has been materialised since the step, or the pass has nothing to read
        bool in_set = ids && n_ids >= 0 && fx_sparse_view(c, agent, &q.set);
        for (int64_t j = 0; in_set && j < n_ids; j++) in_set = ids[j] >= 0 && ids[j] < s.C;
        if (!in_set || !fx_sparse_positions(q.set, n_ids, ids, q.pos))
            return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_BUNDLE");
    }
    if (!params || (detail && !have_out)) return set_err(FX_ERR_INVALID_ARGUMENT, detail ? "params or out is NULL" : "params is NULL");
    const FxRiskParams &p = *params;
    if (p.prob_mode != FX_RISK_PROB_MVN && p.prob_mode != FX_RISK_PROB_MAHALANOBIS)
        return set_err(FX_ERR_INVALID_ARGUMENT, "prob_mode %d", p.prob_mode);
    if ((p.prot_model != FX_RISK_HARM_LOGISTIC && p.prot_model != FX_RISK_HARM_REF_SPEED) ||
        (p.unprot_ego_model != FX_RISK_HARM_LOGISTIC && p.unprot_ego_model != FX_RISK_HARM_REF_SPEED))
        return set_err(FX_ERR_INVALID_ARGUMENT, "harm model (%d, %d)", p.prot_model, p.unprot_ego_model);
    if (p.n_edges < 0 || p.n_edges > FX_RISK_MAX_EDGES || (p.prot_model == FX_RISK_HARM_REF_SPEED && p.n_edges != 0))
        return set_err(FX_ERR_INVALID_ARGUMENT, "n_edges %d", p.n_edges);
    if (!(p.ego_mass > 0.0) || !(p.ego_length > 0.0) || !(p.ego_width > 0.0))
        return set_err(FX_ERR_INVALID_ARGUMENT, "ego length / width / mass must be positive");
    FX_TRY(fx_check_id_list(n_ids, ids, "n_ids"));
    if (!have_out) return set_err(FX_ERR_INVALID_ARGUMENT, "an output pointer is NULL");
    FX_TRY(fx_check_id_range(n_ids, ids, s.C));
    FxRiskState *r = risk_state(c);
    const FxRiskAgent &a = r->agents[agent];
    const int S = s.S, K = a.K;
    const bool maha = p.prob_mode == FX_RISK_PROB_MAHALANOBIS;
    if (maha && K > 0 && !a.have_inv) return set_err(FX_ERR_INVALID_ARGUMENT, "Mahalanobis mode needs the inverse covariances");
    for (int k = 0; k < K; k++) {
        const int np = a.n_pos[k];
        if (detail && std::min(S - 1, np) <= 0)
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: min(S - 1, len(pos_list)) == 0 (calc_risk takes the maximum of an empty "
                           "list upstream)", k);
        if (a.n_yaw[k] < std::min(S, np) || (need_v && a.n_v[k] < std::min(S - 1, np)))
            return need_v ? set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: orientation_list (%d) / v_list (%d) shorter than calc_risk indexes "
                                    "(%d / %d)", k, a.n_yaw[k], a.n_v[k], std::min(S, np), std::min(S - 1, np))
                          : set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: orientation_list (%d) shorter than get_collision_probability_fast "
                                    "indexes (%d)", k, a.n_yaw[k], std::min(S, np));
    }
    q.c = c, q.agent = agent, q.s = &s, q.r = r, q.a = &a, q.prm = params;
    q.S = S, q.K = K, q.P = a.P > 0 ? a.P : 1, q.maha = maha;
    q.n = ids ? n_ids : s.C, q.ids = ids;
    q.planes = q.sparse ? q.set.planes : c->h_probs[agent].planes;
    q.ld = q.sparse ? q.set.ld : s.ld;
    q.flags = q.sparse ? q.set.flags : c->d_flags + s.cand_off;
    q.bstep = q.sparse ? q.set.bound_step : c->d_bstep + s.cand_off;
    return FX_OK;
}

// Steps per chunk of the risk items (fx_item_chunk_steps, fx_pass.h), or what fx_risk_items_set_chunk_steps forces (tests: the
// results do not depend on it)
static std::atomic<int> fx_risk_items_chunk_forced{0};
extern "C" void fx_risk_items_set_chunk_steps(int32_t steps) { fx_risk_items_chunk_forced.store(steps > 0 ? steps : 0, std::memory_order_relaxed); }
extern "C" int32_t fx_risk_items_chunk_steps(int64_t n, int32_t S, int32_t K) {
    return fx_item_chunk_steps(n, S, K, fx_risk_items_chunk_forced.load(std::memory_order_relaxed));
}

// The device block of a pass and the uploads every pass makes.  One grow-only allocation, every part 256-byte aligned; the plain
// pass takes no room for the detail pass's columns, and only a pass with cost parameters for their outputs and tables.
// pp_nb > 0: the prediction-probability pass with batches of pp_nb candidates -- room for its per-step scratch and outputs.
// Every other pass has a walk -- room for the partials of one batch of its items (fx_item_batch, fx_pass.h) and for the call's
// parameters; need: the flags a candidate needs when no ids are given.  resp: the responsibility pass -- room for its outputs.
static int risk_stage(RiskPass &q, bool detail, const FxRiskCostParams *cost, size_t pp_nb = 0,
                      uint32_t need = FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED, bool resp = false) {
    FxContext *c = q.c;
    FxRiskState *r = q.r;
    const FxRiskAgent &a = *q.a;
    build_records(a, q.S, q.maha, q.rec);
    const size_t n1 = (size_t)std::max<int64_t>(q.n, 1), K = (size_t)q.K, KP = K * q.P;
    FxBlockLayout lay;
    q.o_rec = lay.take(sizeof(double) * q.rec.size()), q.o_obs = lay.take(sizeof(double) * a.obs.size());
    q.o_pos = lay.take(sizeof(double) * 2 * KP), q.o_yaw = lay.take(sizeof(double) * KP), q.o_v = lay.take(sizeof(double) * KP);
    q.o_ids = lay.take(sizeof(int64_t) * n1), q.o_ego = lay.take(sizeof(double) * n1), q.o_obst = lay.take(sizeof(double) * n1);
    q.o_idx = lay.take(2 * sizeof(long long));
    if (detail) q.o_occ = lay.take(sizeof(double) * n1), q.o_col = lay.take(sizeof(double) * 4 * K * n1);
    if (cost) {
        const bool reach = cost->responsibility_mode == FX_RISK_RESP_REACH_SET;
        const size_t nE = q.nE = reach ? a.rs_obs.size() : 0, nP = q.nP = reach ? a.rs_step.size() : 0;
        const size_t nV = q.nV = reach ? a.rs_verts.size() / 2 : 0;
        q.o_out = lay.take(sizeof(double) * 7 * n1), q.o_bh = lay.take(sizeof(double) * n1), q.o_resp = lay.take(sizeof(double) * K);
        q.o_eobs = lay.take(sizeof(int32_t) * nE), q.o_eoff = lay.take(sizeof(int32_t) * (nE + 1));
        q.o_pst = lay.take(sizeof(int32_t) * nP), q.o_voff = lay.take(sizeof(int32_t) * (nP + 1)), q.o_vert = lay.take(sizeof(double) * 2 * nV);
    }
    if (pp_nb) {
        q.o_pstep = lay.take(sizeof(double) * K * (size_t)std::max(q.S - 1, 1) * pp_nb);
        q.o_pprob = lay.take(sizeof(double) * n1), q.o_pobs = lay.take(sizeof(double) * K * n1), q.o_ptot = lay.take(sizeof(double) * n1);
        q.o_pbest = lay.take(2 * sizeof(long long));
    }
    const bool walk = pp_nb == 0;
    if (walk) {
        const size_t steps = (size_t)std::max(q.S - 1, 1), nv = detail ? 7 : 2;
        q.it.cs = fx_risk_items_chunk_steps(q.n, q.S, q.K);
        q.it.chunks = (int32_t)((steps + q.it.cs - 1) / q.it.cs);
        const size_t per_cand = sizeof(double) * nv * std::max<size_t>(K, 1) * (size_t)q.it.chunks;
        q.it.nb = fx_item_batch(per_cand, q.n);
        q.it.need = need;
        q.o_part = lay.take(per_cand * (size_t)q.it.nb), q.o_prm = lay.take(sizeof(FxRiskParams));
    }
    if (resp) {
        q.o_rresp = lay.take(sizeof(double) * n1), q.o_rtot = lay.take(sizeof(double) * n1), q.o_rpred = lay.take(sizeof(double) * n1);
        q.o_rbest = lay.take(2 * sizeof(long long));
    }
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(lay.size()));
    FX_TRY(r->ev.ensure());
    q.base = r->block;
    if (walk) {
        q.it.part = q.D(q.o_part);
        q.it.params = reinterpret_cast<const FxRiskParams *>(q.base + q.o_prm);
    }
    if (q.K > 0) {   // (without an obstacle no kernel reads any of these)
        if (walk) HIP_TRY(q.up(q.o_prm, q.prm, sizeof(FxRiskParams)));
        HIP_TRY(q.up(q.o_rec, q.rec.data(), sizeof(double) * q.rec.size()));
        HIP_TRY(q.up(q.o_obs, a.obs.data(), sizeof(double) * a.obs.size()));
        HIP_TRY(q.up(q.o_pos, a.pos.data(), sizeof(double) * a.pos.size()));
        HIP_TRY(q.up(q.o_yaw, a.yaw.data(), sizeof(double) * a.yaw.size()));
        HIP_TRY(q.up(q.o_v, a.v.data(), sizeof(double) * a.v.size()));
    }
    if (q.ids && q.n > 0) HIP_TRY(q.up(q.o_ids, q.sparse ? q.pos.data() : q.ids, sizeof(int64_t) * q.n));
    return FX_OK;
}

// The launches of a pass (fx_launch_risk), the read-back of what the caller asked for, and the device time
static int risk_run(RiskPass &q, bool detail, const RiskCostArgs *ca, const FxRiskOutputs &out, const RespSumArgs *rs = nullptr) {
    FxContext *c = q.c;
    FxRiskState *r = q.r;
    const RiskWalkArgs w{q.planes, q.ld, q.S, q.n, q.d_ids(), q.flags, q.D(q.o_rec), q.D(q.o_obs),
                         q.D(q.o_pos), q.D(q.o_yaw), q.D(q.o_v), q.K, q.P};
    long long *d_idx = reinterpret_cast<long long *>(q.base + q.o_idx);
    HIP_TRY(fx_launch_risk(&w, &q.it, q.D(q.o_ego), q.D(q.o_obst), detail ? q.D(q.o_col) : nullptr, detail ? q.D(q.o_occ) : nullptr, ca, d_idx,
                           r->ev.e0, r->ev.e1, c->stream, rs,
                           rs ? reinterpret_cast<long long *>(q.base + q.o_rbest) : nullptr));
    const size_t nn = (size_t)q.n, Kn = (size_t)q.K * nn;
    HIP_TRY(q.down(out.ego_risk, q.o_ego, nn));
    HIP_TRY(q.down(out.obst_risk, q.o_obst, nn));
    if (detail) {
        HIP_TRY(q.down(out.obst_harm_occ, q.o_occ, nn));
        double *const cols[4] = {out.ego_risk_max, out.obst_risk_max, out.ego_harm_max, out.obst_harm_max};
        for (int k = 0; k < 4; k++) HIP_TRY(q.down(cols[k], q.o_col + sizeof(double) * k * Kn, Kn));
    }
    if (ca) {
        double *const pr[7] = {out.bayes, out.equality, out.maximin, out.ego, out.responsibility, out.total, out.boundary_harm};
        for (int k = 0; k < 7; k++) {
            if (rs && (k == 4 || k == 5)) continue;   // (the responsibility pass answers these two from its own sum, below)
            HIP_TRY(q.down(pr[k], q.o_out + sizeof(double) * k * nn, nn));
        }
    }
    if (rs) {
        HIP_TRY(q.down(out.responsibility, q.o_rresp, nn));
        HIP_TRY(q.down(out.total, q.o_rtot, nn));
    }
    long long idx[2] = {-1, -1};   // (the second one: the cost pass's arg-min)
    HIP_TRY(hipMemcpyAsync(idx, d_idx, sizeof(long long) * (ca ? 2 : 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->ev.e0, r->ev.e1));
    // (sparse set: the arg-min ran over positions, which grow with the candidate index -- the same winner, the same tie rule)
    for (long long &i : idx)
        if (q.sparse && i >= 0) i = (long long)q.set.ids[i];
    if (out.min_risk_index) *out.min_risk_index = (int64_t)idx[0];
    if (out.min_cost_index) *out.min_cost_index = (int64_t)idx[1];
    return FX_OK;
}

extern "C" int32_t fx_eval_risk_agent(FxContext *c, int32_t agent, const FxRiskParams *params, int64_t n_ids, const int64_t *ids,
                                      double *ego_risk, double *obst_risk, int64_t *min_risk_index) {
    RiskPass q;
    int rc = risk_check(q, c, agent, params, n_ids, ids, ego_risk && obst_risk && min_risk_index, false);
    if (rc || (rc = risk_stage(q, false, nullptr))) return rc;
    FxRiskOutputs out{};
    out.ego_risk = ego_risk, out.obst_risk = obst_risk, out.min_risk_index = min_risk_index;
    return risk_run(q, false, nullptr, out);
}

extern "C" int32_t fx_set_reach_sets_agent(FxContext *c, int32_t agent, int32_t n_entries, const int32_t *entry_obs,
                                           const int32_t *entry_part_off, int32_t n_parts, const int32_t *part_step,
                                           const int32_t *part_vert_off, int32_t n_verts, const double *verts) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (agent < 0 || agent >= c->max_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
    if (n_entries < 0 || n_parts < 0 || n_verts < 0 || (n_entries > 0 && (!entry_obs || !entry_part_off)) ||
        (n_parts > 0 && (n_entries == 0 || !part_step || !part_vert_off || !verts)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "reach-set arrays inconsistent (entries=%d, parts=%d, vertices=%d)", n_entries, n_parts, n_verts);
    if (n_entries > 0) {
        if (entry_part_off[0] != 0 || entry_part_off[n_entries] != n_parts)
            return set_err(FX_ERR_INVALID_ARGUMENT, "entry_part_off must run from 0 to n_parts=%d", n_parts);
        for (int e = 0; e < n_entries; e++) {
            if (entry_part_off[e + 1] < entry_part_off[e]) return set_err(FX_ERR_INVALID_ARGUMENT, "entry_part_off decreases at entry %d", e);
            if (entry_obs[e] < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "entry %d: obstacle index %d", e, entry_obs[e]);
        }
    }
    if (n_parts > 0) {
        if (part_vert_off[0] != 0 || part_vert_off[n_parts] != n_verts)
            return set_err(FX_ERR_INVALID_ARGUMENT, "part_vert_off must run from 0 to n_verts=%d", n_verts);
        for (int p = 0; p < n_parts; p++) {
            if (part_vert_off[p + 1] - part_vert_off[p] < 3)
                return set_err(FX_ERR_INVALID_ARGUMENT, "part %d: a polygon needs at least 3 vertices", p);
            if (part_step[p] < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "part %d: step index %d", p, part_step[p]);
        }
    }
    FxRiskAgent &a = risk_state(c)->agents[agent];
    a.rs_obs.assign(entry_obs, entry_obs + n_entries);
    a.rs_off.clear();
    if (n_entries > 0) a.rs_off.assign(entry_part_off, entry_part_off + n_entries + 1);
    a.rs_step.assign(part_step, part_step + n_parts);
    a.rs_voff.clear();
    if (n_parts > 0) a.rs_voff.assign(part_vert_off, part_vert_off + n_parts + 1);
    a.rs_verts.assign(verts, verts + 2 * (size_t)n_verts);
    return FX_OK;
}

// the checks of a cost pass's parameters against the agent's obstacles, reach sets and horizon
static int risk_cost_check(const RiskPass &q, const FxRiskCostParams *cost) {
    const FxRiskAgent &a = *q.a;
    const int S = q.S, K = q.K;
    if (cost->boundary_mode < FX_RISK_BOUNDARY_ZERO || cost->boundary_mode > FX_RISK_BOUNDARY_STEP ||
        (cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY && !cost->boundary_harm))
        return set_err(FX_ERR_INVALID_ARGUMENT, "boundary_mode %d", cost->boundary_mode);
    if (cost->responsibility_mode < FX_RISK_RESP_NONE || cost->responsibility_mode > FX_RISK_RESP_REACH_SET ||
        (cost->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && K > 0 && !cost->responsibility))
        return set_err(FX_ERR_INVALID_ARGUMENT, "responsibility_mode %d", cost->responsibility_mode);
    if (cost->responsibility_mode == FX_RISK_RESP_REACH_SET) {
        for (size_t e = 0; e < a.rs_obs.size(); e++)
            if (a.rs_obs[e] >= K)
                return set_err(FX_ERR_INVALID_ARGUMENT, "reach-set entry %d: obstacle index %d is not among the %d predictions", (int)e,
                               a.rs_obs[e], K);
        for (size_t t = 0; t < a.rs_step.size(); t++)
            if (a.rs_step[t] >= S)
                return set_err(FX_ERR_INVALID_ARGUMENT, "reach-set part %d: step index %d outside the horizon (S=%d)", (int)t, a.rs_step[t], S);
    }
    return FX_OK;
}

// the argument block of a cost pass's kernel from where the pass's parts lie (q.base, q.o_*): no HIP call
static void risk_cost_fill(const RiskPass &q, const FxRiskCostParams *cost, RiskCostArgs &ca);

// the uploads of a staged cost pass and the argument block of its kernel
static int risk_cost_args(const RiskPass &q, const FxRiskCostParams *cost, RiskCostArgs &ca) {
    const FxRiskAgent &a = *q.a;
    const int K = q.K;
    const int64_t n = q.n;
    const size_t nE = q.nE, nP = q.nP, nV = q.nV;
    if (cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY && n > 0) HIP_TRY(q.up(q.o_bh, cost->boundary_harm, sizeof(double) * n));
    if (cost->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && K > 0) HIP_TRY(q.up(q.o_resp, cost->responsibility, sizeof(double) * K));
    if (nE > 0) {
        HIP_TRY(q.up(q.o_eobs, a.rs_obs.data(), sizeof(int32_t) * nE));
        HIP_TRY(q.up(q.o_eoff, a.rs_off.data(), sizeof(int32_t) * (nE + 1)));
        if (nP > 0) {
            HIP_TRY(q.up(q.o_pst, a.rs_step.data(), sizeof(int32_t) * nP));
            HIP_TRY(q.up(q.o_voff, a.rs_voff.data(), sizeof(int32_t) * (nP + 1)));
            HIP_TRY(q.up(q.o_vert, a.rs_verts.data(), sizeof(double) * 2 * nV));
        }
    }
    risk_cost_fill(q, cost, ca);
    return FX_OK;
}

static void risk_cost_fill(const RiskPass &q, const FxRiskCostParams *cost, RiskCostArgs &ca) {
    const FxAgentSlot &s = *q.s;
    const int S = q.S, K = q.K;
    const int64_t n = q.n;
    const size_t nE = q.nE;
    ca.col = q.D(q.o_col);
    ca.n = n;
    ca.ids = q.d_ids();
    ca.flags = q.flags;
    ca.planes = q.planes;
    ca.ld = q.ld;
    ca.S = S;
    ca.K = K;
    ca.bh_in = cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY ? q.D(q.o_bh) : nullptr;
    ca.bstep = (cost->boundary_mode == FX_RISK_BOUNDARY_STEP && (s.mode & FX_MODE_ROAD_BOUNDARY)) ? q.bstep : nullptr;
    ca.bh_c = cost->boundary_c;
    ca.bh_s = cost->boundary_s;
    ca.resp_mode = cost->responsibility_mode;
    ca.n_entries = (int32_t)nE;
    ca.resp = q.D(q.o_resp);
    ca.entry_obs = q.I(q.o_eobs);
    ca.entry_off = q.I(q.o_eoff);
    ca.part_step = q.I(q.o_pst);
    ca.vert_off = q.I(q.o_voff);
    ca.verts = q.D(q.o_vert);
    for (int k = 0; k < 5; k++) ca.w[k] = cost->weights[k];
    ca.eps = cost->maximin_eps;
    ca.scale = cost->maximin_scale;
    ca.out = q.D(q.o_out);
}

extern "C" int32_t fx_eval_risk_costs_agent(FxContext *c, int32_t agent, const FxRiskParams *params, const FxRiskCostParams *cost,
                                            int64_t n_ids, const int64_t *ids, const FxRiskOutputs *out) {
    RiskPass q;
    int rc = risk_check(q, c, agent, params, n_ids, ids, out != nullptr, true);
    if (rc) return rc;
    if (cost) FX_TRY(risk_cost_check(q, cost));
    if ((rc = risk_stage(q, true, cost))) return rc;
    RiskCostArgs ca{};
    if (cost) FX_TRY(risk_cost_args(q, cost, ca));
    return risk_run(q, true, cost ? &ca : nullptr, *out);
}

// The responsibility cost as a weighted term of the step's cost (fxplan.h): the detail pass, the
// responsibility part of the cost pass over its columns, and the re-sum with its arg-min.
// The checks of the responsibility pass for one agent, in the order the entry points report them (the per-agent call and the
// batched one); cost: the cost pass with the responsibility alone -- no boundary harm, total = the responsibility cost
static int resp_check(RiskPass &q, FxContext *c, int32_t agent, const FxRiskParams *params, const FxRespCostParams *resp, int64_t n_ids,
                      const int64_t *ids, bool have_out, FxRiskCostParams &cost) {
    FX_TRY(check_agent(c, agent));
    if (!fx_inputs_current(c))   // (the condition of fx_eval_prediction_prob_agent: the planes and cost rows are the last evaluated step's)
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    if (!(c->slots[agent].mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_COSTMAP");
    FX_TRY(risk_check(q, c, agent, (params && resp) ? params : nullptr, n_ids, ids, have_out, true));
    if (!(resp->weight != 0.0) || resp->weight != resp->weight) return set_err(FX_ERR_INVALID_ARGUMENT, "responsibility weight %g", resp->weight);
    if (resp->responsibility_mode != FX_RISK_RESP_ACTION_SPACE && resp->responsibility_mode != FX_RISK_RESP_REACH_SET)
        return set_err(FX_ERR_INVALID_ARGUMENT, "responsibility_mode %d", resp->responsibility_mode);
    cost = FxRiskCostParams{};
    cost.weights[4] = 1.0;
    cost.maximin_scale = 1.0;
    cost.boundary_mode = FX_RISK_BOUNDARY_ZERO;
    cost.responsibility_mode = resp->responsibility_mode;
    cost.responsibility = resp->responsibility;
    return risk_cost_check(q, &cost);
}

// what the re-sum reads of a checked agent's cost list, but for the pointers into the pass's block
static void resp_sum_fill(const RiskPass &q, const FxRespCostParams *resp, RespSumArgs &rs) {
    const DevProblem &hp = q.c->h_probs[q.agent];
    rs.n_pred = -1;
    rs.at = hp.n_cost;   // in front of the first name behind "responsibility" in the sorted list
    for (int m = hp.n_cost - 1; m >= 0; m--) {
        if (hp.cost_id[m] == FX_COST_PREDICTION) rs.n_pred = m;
        if (hp.cost_id[m] > FX_COST_PREDICTION) rs.at = m;
    }
    rs.n = q.n, rs.flags = q.flags, rs.need = FX_FLAG_COSTED;
    rs.costmap = q.sparse ? q.set.costmap : q.c->d_costmap + (size_t)FX_NUM_COSTS * q.s->cand_off;
    rs.ld = q.ld;
    rs.n_cost = hp.n_cost;
    // (a sparse set's rows were closed by the list kernel, which never defers)
    rs.deferred = (!q.sparse && (hp.mode & FX_MODE_INT_DEFER_OBST)) ? 1 : 0;
    for (int m = 0; m < hp.n_cost; m++) rs.cost_w[m] = hp.cost_w[m];
    rs.w_resp = resp->weight;
}

extern "C" int32_t fx_eval_responsibility_cost_agent(FxContext *c, int32_t agent, const FxRiskParams *params, const FxRespCostParams *resp,
                                                     int64_t n_ids, const int64_t *ids, const FxRespCostOutputs *out) {
    RiskPass q;
    FxRiskCostParams cost;
    FX_TRY(resp_check(q, c, agent, params, resp, n_ids, ids,
                      out && out->resp && out->total && out->ego_risk && out->obst_risk && out->best_index && out->best_cost, cost));
    RespSumArgs rs{};
    resp_sum_fill(q, resp, rs);
    const uint32_t need = FX_FLAG_COSTED;
    FX_TRY(risk_stage(q, true, &cost, 0, need, true));
    RiskCostArgs ca{};
    FX_TRY(risk_cost_args(q, &cost, ca));
    if (!q.ids && q.n > 0) {
        // every candidate: the cost kernel's own rule for that (VALID, FEASIBLE and RETURNED) is not this pass's (COSTED), so it gets
        // the identity list and evaluates every row; the rows of candidates without a cost are NaN columns in, NaN out, never read
        std::vector<int64_t> all((size_t)q.n);
        for (int64_t j = 0; j < q.n; j++) all[(size_t)j] = j;
        HIP_TRY(q.up(q.o_ids, all.data(), sizeof(int64_t) * all.size()));
        HIP_TRY(hipStreamSynchronize(c->stream));   // (the list is a local)
        ca.ids = reinterpret_cast<const int64_t *>(q.base + q.o_ids);
    }
    if (resp->prediction && q.n > 0) HIP_TRY(q.up(q.o_rpred, resp->prediction, sizeof(double) * q.n));
    rs.ids = q.d_ids();
    rs.resp = q.D(q.o_out) + 4 * (size_t)q.n;
    rs.pred = (resp->prediction && rs.n_pred >= 0) ? q.D(q.o_rpred) : nullptr;
    rs.resp_out = q.D(q.o_rresp), rs.total = q.D(q.o_rtot);
    FxRiskOutputs ro{};
    ro.ego_risk = out->ego_risk, ro.obst_risk = out->obst_risk, ro.responsibility = out->resp, ro.total = out->total;
    FX_TRY(risk_run(q, true, &ca, ro, &rs));
    long long best[2] = {-1, 0};
    HIP_TRY(hipMemcpy(best, q.base + q.o_rbest, sizeof(best), hipMemcpyDeviceToHost));
    // (sparse set: the arg-min ran over positions, which grow with the candidate index -- the same winner, the same tie rule)
    if (q.sparse && best[0] >= 0) best[0] = (long long)q.set.ids[best[0]];
    *out->best_index = (int64_t)best[0];
    memcpy(out->best_cost, &best[1], sizeof(double));
    return FX_OK;
}

// Collision probability as the prediction cost (fxplan.h).  The scratch holds the per-step probabilities of
// one batch of candidates, [K][S - 1][batch] (fx_item_batch, fx_pass.h).
// The checks of the pass for one agent, in the order the entry points report them; n_pred: where the cost list has its prediction
static int predprob_check(RiskPass &q, FxContext *c, int32_t agent, const FxPredProbParams *params, int64_t n_ids, const int64_t *ids,
                          bool have_out, int &n_pred) {
    FX_TRY(check_agent(c, agent));
    // (the planes and the cost map are the last EVALUATED step's: inputs rewritten since belong to a step that has not run -- the
    // condition of the sort and of the sparse set, fx_api_sort.hip / fx_api_materialise.hip)
    if (!fx_inputs_current(c))   // (check_agent has established `evaluated`)
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    if (!(c->slots[agent].mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_COSTMAP");
    FxRiskParams rp{};   // what risk_check and step_probability read of it: the MVN mode and the ego's footprint
    rp.prob_mode = FX_RISK_PROB_MVN;
    rp.prot_model = rp.unprot_ego_model = FX_RISK_HARM_LOGISTIC;
    rp.ego_mass = 1.0;
    if (params) { rp.ego_length = params->ego_length; rp.ego_width = params->ego_width; }
    FX_TRY(risk_check(q, c, agent, params ? &rp : nullptr, n_ids, ids, have_out, false, false));
    q.prm = nullptr;   // (rp is a local; this pass reads the footprint from its own parameters)
    if (params->source != FX_PRED_SOURCE_PROBABILITY && params->source != FX_PRED_SOURCE_STEP)
        return set_err(FX_ERR_INVALID_ARGUMENT, "source %d", params->source);
    const DevProblem &hp = c->h_probs[agent];
    n_pred = -1;
    for (int m = 0; m < hp.n_cost; m++)
        if (hp.cost_id[m] == FX_COST_PREDICTION) n_pred = m;
    if (n_pred < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "the cost list has no FX_COST_PREDICTION");
    return FX_OK;
}

// what the kernels read of a checked agent, but for the records, the scratch and the outputs
static void predprob_args(const RiskPass &q, const FxPredProbParams *params, int n_pred, PredProbArgs &a) {
    const DevProblem &hp = q.c->h_probs[q.agent];
    a.planes = q.planes, a.ld = q.ld, a.S = q.S, a.K = q.K, a.n = q.n, a.flags = q.flags;
    a.ego_length = params->ego_length, a.ego_width = params->ego_width, a.source = params->source;
    a.costmap = q.sparse ? q.set.costmap : q.c->d_costmap + (size_t)FX_NUM_COSTS * q.s->cand_off;
    a.n_cost = hp.n_cost, a.n_pred = n_pred;
    // (a sparse set's rows were closed by the list kernel, which never defers)
    a.deferred = (!q.sparse && (hp.mode & FX_MODE_INT_DEFER_OBST)) ? 1 : 0;
    for (int m = 0; m < hp.n_cost; m++) a.cost_w[m] = hp.cost_w[m];
}

extern "C" int32_t fx_eval_prediction_prob_agent(FxContext *c, int32_t agent, const FxPredProbParams *params, int64_t n_ids,
                                                 const int64_t *ids, const FxPredProbOutputs *out) {
    RiskPass q;
    int n_pred;
    FX_TRY(predprob_check(q, c, agent, params, n_ids, ids, out != nullptr, n_pred));
    const size_t per_cand = sizeof(double) * (size_t)std::max(q.K, 1) * (size_t)std::max(q.S - 1, 1);
    const size_t nb = (size_t)fx_item_batch(per_cand, q.n);
    FX_TRY(risk_stage(q, false, nullptr, nb));
    FxRiskState *r = q.r;
    PredProbArgs a{};
    predprob_args(q, params, n_pred, a);
    a.ids = q.d_ids(), a.rec = q.D(q.o_rec);
    a.step = q.D(q.o_pstep), a.nb = (int64_t)nb;
    a.prob = q.D(q.o_pprob), a.prob_obs = out->prob_obs ? q.D(q.o_pobs) : nullptr, a.total = q.D(q.o_ptot);
    long long *d_best = reinterpret_cast<long long *>(q.base + q.o_pbest);
    HIP_TRY(fx_launch_predprob(&a, d_best, r->ev.e0, r->ev.e1, c->stream));
    const size_t nn = (size_t)q.n;
    HIP_TRY(q.down(out->prob, q.o_pprob, nn));
    HIP_TRY(q.down(out->prob_obs, q.o_pobs, (size_t)q.K * nn));
    HIP_TRY(q.down(out->total, q.o_ptot, nn));
    long long best[2] = {-1, 0};
    HIP_TRY(hipMemcpyAsync(best, d_best, sizeof(best), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_pp_ms, r->ev.e0, r->ev.e1));
    // (sparse set: the arg-min ran over positions, which grow with the candidate index -- the same winner, the same tie rule)
    if (q.sparse && best[0] >= 0) best[0] = (long long)q.set.ids[best[0]];
    if (out->best_index) *out->best_index = (int64_t)best[0];
    if (out->best_cost) memcpy(out->best_cost, &best[1], sizeof(double));
    return FX_OK;
}

// The same pass over every candidate of several agents in ONE call (fxplan.h).  Per agent the checks and
// records of the call above; then all records and all tables in one staging buffer each, the rounds of fx_item_rounds (fx_pass.h)
// over one scratch, and per round two launches whatever the agent count.  Runtime calls of a call with R rounds: 1 drain
// (a synchronisation), 2 copies up (records, tables), 2 event records, 2 R + 1 launches, 3 copies down (prob, total, best),
// 1 synchronisation -- none of them per agent.
static std::atomic<long long> fx_predprob_scratch_forced{0};
extern "C" void fx_predprob_set_scratch_limit(int64_t bytes) { fx_predprob_scratch_forced.store(bytes > 0 ? bytes : 0, std::memory_order_relaxed); }

extern "C" int32_t fx_eval_prediction_prob_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxPredProbParams *params,
                                                 const FxPredProbBatchOutputs *out) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!params || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "params or out is NULL");
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    if (!fx_launch_predprob_batch || !fx_predprob_chunk_steps) return set_err(FX_ERR_HIP, "built without the batched prediction-probability launcher");
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "no evaluated plan step");
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d of %d uploaded agents", n_agents, c->n_agents);
    const size_t A = (size_t)n_agents;
    std::vector<RiskPass> q(A);
    std::vector<int> n_pred(A);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (size_t i = 0; i < A; i++) {
        const int32_t agent = agents ? agents[i] : (int32_t)i;
        if (agent >= 0 && agent < c->n_agents && listed[agent]) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        if (const int rc = predprob_check(q[i], c, agent, params + i, 0, nullptr, true, n_pred[i])) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return set_err(rc, "agent %d: %s", agent, why);
        }
        listed[agent] = 1;
    }
    // records of all agents in one buffer; one candidate's share of the scratch: a probability per (obstacle, step), none where
    // no item runs
    std::vector<double> rec, one;
    std::vector<size_t> rec_at(A), out_at(A);
    std::vector<FxItemAgent> ia(A);
    size_t rows_out = 0;
    for (size_t i = 0; i < A; i++) {
        const RiskPass &p = q[i];
        rec_at[i] = rec.size();
        out_at[i] = rows_out;
        rows_out += (size_t)p.n;
        const bool items = params[i].source == FX_PRED_SOURCE_PROBABILITY && p.K > 0 && p.S > 1;
        if (items) {
            build_records(*p.a, p.S, false, one);
            rec.insert(rec.end(), one.begin(), one.end());
        }
        ia[i] = FxItemAgent{p.n, items ? sizeof(double) * (size_t)p.K * (size_t)(p.S - 1) : 0};
    }
    const long long forced = fx_predprob_scratch_forced.load(std::memory_order_relaxed);
    const size_t limit = forced > 0 ? (size_t)forced : FX_ITEM_SCRATCH_BYTES;
    const std::vector<FxItemSegment> segs = fx_item_rounds(ia.data(), n_agents, limit);
    const size_t R = segs.size();
    const int n_rounds = R ? segs.back().round + 1 : 0;
    // the rounds' sizes: tiles x obstacles of all rows choose the chunk steps of each (fx_item_chunk_steps), the largest scratch
    std::vector<PredProbRound> rounds((size_t)n_rounds, PredProbRound{0, 0, 0, 0});
    std::vector<int64_t> tile_obst((size_t)n_rounds, 0);
    size_t scratch = 0;
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const size_t tiles = (size_t)(g.count + 63) / 64;
        if (ia[g.agent].per_candidate_bytes) tile_obst[g.round] += (int64_t)tiles * q[g.agent].K;
        scratch = std::max(scratch, g.scratch_off + tiles * 64 * ia[g.agent].per_candidate_bytes);
    }
    FxBlockLayout lay;
    const size_t o_rec = lay.take(sizeof(double) * rec.size());
    const size_t t_rows = 0, t_item0 = align_up(sizeof(PredProbRow) * R, 8), t_fin0 = t_item0 + sizeof(int64_t) * R,
                 t_arow = t_fin0 + sizeof(int32_t) * R, t_size = t_arow + sizeof(int32_t) * A;
    const size_t o_tab = lay.take(t_size), o_step = lay.take(scratch);
    const size_t o_prob = lay.take(sizeof(double) * rows_out), o_tot = lay.take(sizeof(double) * rows_out);
    const size_t o_best = lay.take(2 * sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(lay.size()));
    FX_TRY(r->ev.ensure());
    char *base = r->block;
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    std::vector<char> tab(t_size, 0);
    PredProbRow *rows = reinterpret_cast<PredProbRow *>(tab.data() + t_rows);
    int64_t *item0 = reinterpret_cast<int64_t *>(tab.data() + t_item0);
    int32_t *fin0 = reinterpret_cast<int32_t *>(tab.data() + t_fin0), *agent_row = reinterpret_cast<int32_t *>(tab.data() + t_arow);
    for (size_t i = 0; i < A; i++) agent_row[i] = -1;
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const RiskPass &p = q[g.agent];
        PredProbRound &rd = rounds[g.round];
        if (rd.n_rows == 0) rd.row0 = (int32_t)k;
        rd.n_rows++;
        PredProbRow &w = rows[k];
        predprob_args(p, params + g.agent, n_pred[g.agent], w.a);
        w.a.ids = nullptr, w.a.rec = D(o_rec) + rec_at[g.agent];
        w.a.step = reinterpret_cast<double *>(base + o_step + g.scratch_off), w.a.nb = (g.count + 63) / 64 * 64;
        w.a.prob = D(o_prob) + out_at[g.agent], w.a.prob_obs = nullptr, w.a.total = D(o_tot) + out_at[g.agent];
        w.first = g.first, w.count = g.count;
        const bool items = ia[g.agent].per_candidate_bytes != 0;
        // (the round's tiles x obstacles as the candidates of ONE obstacle: the rule then sees the launch, not the agent)
        w.cs = fx_predprob_chunk_steps(64 * tile_obst[g.round], p.S, 1);
        w.chunks = items ? (std::max(p.S - 1, 1) + w.cs - 1) / w.cs : 0;
        w.item0 = item0[k] = rd.items;
        w.fin0 = fin0[k] = rd.fin_blocks;
        rd.items += (w.a.nb / 64) * w.chunks * (int64_t)p.K;
        rd.fin_blocks += (int32_t)((g.count + 255) / 256);
        agent_row[g.agent] = (int32_t)k;
    }
    for (const PredProbRound &rd : rounds)
        if (rd.items > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld items", (long long)rd.items);
    if (!rec.empty()) HIP_TRY(hipMemcpyAsync(base + o_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(base + o_tab, tab.data(), t_size, hipMemcpyHostToDevice, c->stream));
    PredProbBatchArgs t{};
    t.rows = reinterpret_cast<const PredProbRow *>(base + o_tab + t_rows);
    t.item0 = reinterpret_cast<const int64_t *>(base + o_tab + t_item0);
    t.fin0 = reinterpret_cast<const int32_t *>(base + o_tab + t_fin0);
    t.agent_row = reinterpret_cast<const int32_t *>(base + o_tab + t_arow);
    t.n_agents = n_agents;
    long long *d_best = reinterpret_cast<long long *>(base + o_best);
    HIP_TRY(fx_launch_predprob_batch(&t, rounds.data(), n_rounds, d_best, r->ev.e0, r->ev.e1, c->stream));
    if (out->prob && rows_out) HIP_TRY(hipMemcpyAsync(out->prob, base + o_prob, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    if (out->total && rows_out) HIP_TRY(hipMemcpyAsync(out->total, base + o_tot, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    std::vector<long long> best(2 * A);
    HIP_TRY(hipMemcpyAsync(best.data(), d_best, sizeof(long long) * 2 * A, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_pp_ms, r->ev.e0, r->ev.e1));
    for (size_t i = 0; i < A; i++) {
        if (out->best_index) out->best_index[i] = (int64_t)best[2 * i];
        if (out->best_cost) memcpy(out->best_cost + i, &best[2 * i + 1], sizeof(double));
    }
    return FX_OK;
}

// The responsibility pass over every candidate of several agents in ONE call (fxplan.h).  Per agent the checks
// of the per-agent entry (resp_check) and its records; then everything the kernels read -- FxRiskParams, records, obstacle tables,
// responsibility vectors, prediction entries, reach-set tables, and the rows, compact arrays and per-agent argument blocks that
// point at them -- in ONE staging buffer and one copy; the rounds of fx_item_rounds over one scratch with each row's steps per
// chunk chosen from its agent's OWN size, as the per-agent call chooses them.  Runtime calls of a call with R rounds: 1 drain (a
// synchronisation), 1 ensure of the block, 1 copy up, 2 event records, 2 R + 3 launches, 5 copies down (resp, total, ego_risk,
// obst_risk, best), 1 synchronisation -- none of them per agent.
static std::atomic<unsigned long long> fx_risk_batch_scratch_forced{0};
extern "C" void fx_risk_batch_set_scratch_limit(size_t bytes) { fx_risk_batch_scratch_forced.store(bytes, std::memory_order_relaxed); }

extern "C" int32_t fx_eval_responsibility_cost_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params,
                                                     const FxRespCostParams *resp, const FxRespCostBatchOutputs *out) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!params || !resp || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "params, resp or out is NULL");
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    if (!fx_launch_risk_batch) return set_err(FX_ERR_HIP, "built without the batched responsibility launcher");
    const int32_t agent0 = agents ? agents[0] : 0;
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "agent %d: no evaluated plan step", agent0);
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d of %d uploaded agents", n_agents, c->n_agents);
    const size_t A = (size_t)n_agents;
    const bool have_out = out->resp && out->total && out->ego_risk && out->obst_risk && out->best_index && out->best_cost;
    std::vector<RiskPass> q(A);
    std::vector<FxRiskCostParams> cost(A);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (size_t i = 0; i < A; i++) {
        const int32_t agent = agents ? agents[i] : (int32_t)i;
        if (agent >= 0 && agent < c->n_agents && listed[agent]) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        if (const int rc = resp_check(q[i], c, agent, params + i, resp + i, 0, nullptr, have_out, cost[i])) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return set_err(rc, "agent %d: %s", agent, why);
        }
        listed[agent] = 1;   // (without ids risk_check has refused a step that stored no bundle)
    }
    // ONE staging buffer, every part 16-byte aligned; the device's copy lies at o_stage of the block
    std::vector<char> stage;
    auto room = [&](size_t bytes) { const size_t o = stage.size(); stage.resize(o + align_up(std::max<size_t>(bytes, 8), 16), 0); return o; };
    auto put = [&](const void *src, size_t bytes) { const size_t o = room(bytes); if (bytes) memcpy(stage.data() + o, src, bytes); return o; };
    struct Parts { size_t prm, rec, obs, pos, yaw, v, resp, pred, eobs, eoff, pst, voff, vert, out_at, col_at; bool items, has_pred; };
    std::vector<Parts> at(A);
    std::vector<RespSumArgs> sums(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<int32_t> cs(A), chunks(A), blk0(A);
    std::vector<double> rec;
    size_t rows_out = 0, col_doubles = 0;
    int64_t blocks = 0;
    for (size_t i = 0; i < A; i++) {
        RiskPass &p = q[i];
        const FxRiskAgent &a = *p.a;
        Parts &t = at[i];
        t = Parts{};
        t.out_at = rows_out, t.col_at = col_doubles;
        rows_out += (size_t)p.n;
        col_doubles += 4 * (size_t)p.K * (size_t)p.n;
        blk0[i] = (int32_t)blocks;
        blocks += (p.n + 255) / 256;
        t.prm = put(p.prm, sizeof(FxRiskParams));
        if (p.K > 0) {
            build_records(a, p.S, p.maha, rec);
            t.rec = put(rec.data(), sizeof(double) * rec.size()), t.obs = put(a.obs.data(), sizeof(double) * a.obs.size());
            t.pos = put(a.pos.data(), sizeof(double) * a.pos.size()), t.yaw = put(a.yaw.data(), sizeof(double) * a.yaw.size());
            t.v = put(a.v.data(), sizeof(double) * a.v.size());
            if (resp[i].responsibility_mode == FX_RISK_RESP_ACTION_SPACE) t.resp = put(resp[i].responsibility, sizeof(double) * p.K);
        }
        if (resp[i].responsibility_mode == FX_RISK_RESP_REACH_SET) {
            p.nE = a.rs_obs.size(), p.nP = a.rs_step.size(), p.nV = a.rs_verts.size() / 2;
            t.eobs = put(a.rs_obs.data(), sizeof(int32_t) * p.nE), t.eoff = put(a.rs_off.data(), sizeof(int32_t) * a.rs_off.size());
            t.pst = put(a.rs_step.data(), sizeof(int32_t) * p.nP), t.voff = put(a.rs_voff.data(), sizeof(int32_t) * a.rs_voff.size());
            t.vert = put(a.rs_verts.data(), sizeof(double) * a.rs_verts.size());
        }
        resp_sum_fill(p, resp + i, sums[i]);
        t.has_pred = resp[i].prediction && sums[i].n_pred >= 0 && p.n > 0;
        if (t.has_pred) t.pred = put(resp[i].prediction, sizeof(double) * (size_t)p.n);
        // steps per chunk from the agent's OWN size: what fx_eval_responsibility_cost_agent chooses for it
        t.items = p.K > 0 && p.S > 1;
        cs[i] = fx_risk_items_chunk_steps(p.n, p.S, p.K);
        chunks[i] = (std::max(p.S - 1, 1) + cs[i] - 1) / cs[i];
        ia[i] = FxItemAgent{p.n, t.items ? sizeof(double) * 7 * (size_t)p.K * (size_t)chunks[i] : 0};
    }
    if (blocks > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "%lld workgroups of candidates", (long long)blocks);
    const unsigned long long forced = fx_risk_batch_scratch_forced.load(std::memory_order_relaxed);
    const std::vector<FxItemSegment> segs = fx_item_rounds(ia.data(), n_agents, forced ? (size_t)forced : FX_ITEM_SCRATCH_BYTES);
    const size_t R = segs.size();
    const int n_rounds = R ? segs.back().round + 1 : 0;
    std::vector<RiskBatchRound> rounds((size_t)n_rounds, RiskBatchRound{0, 0, 0, 0});
    const size_t t_rows = room(sizeof(RiskBatchRow) * R), t_item0 = room(sizeof(int64_t) * R), t_fin0 = room(sizeof(int32_t) * R),
                 t_cost = room(sizeof(RiskCostArgs) * A), t_sum = room(sizeof(RespSumArgs) * A), t_blk0 = put(blk0.data(), sizeof(int32_t) * A);
    size_t scratch = 0;
    for (size_t k = 0; k < R; k++) {   // the rows' counts (their pointers follow when the block is there)
        const FxItemSegment &g = segs[k];
        const size_t tiles = (size_t)(g.count + 63) / 64;
        RiskBatchRound &rd = rounds[g.round];
        RiskBatchRow w{};
        if (rd.n_rows == 0) rd.row0 = (int32_t)k;
        rd.n_rows++;
        w.first = g.first, w.count = g.count;
        w.it.nb = (int64_t)tiles * 64, w.it.cs = cs[g.agent], w.it.chunks = chunks[g.agent], w.it.need = FX_FLAG_COSTED;
        w.items = at[g.agent].items ? 1 : 0;
        w.item0 = rd.items;
        w.fin0 = rd.fin_blocks;
        if (w.items) rd.items += (int64_t)tiles * chunks[g.agent] * (int64_t)q[g.agent].K;
        rd.fin_blocks += (int32_t)((g.count + 255) / 256);
        scratch = std::max(scratch, g.scratch_off + tiles * 64 * ia[g.agent].per_candidate_bytes);
        memcpy(stage.data() + t_rows + sizeof(RiskBatchRow) * k, &w, sizeof(w));
        memcpy(stage.data() + t_item0 + sizeof(int64_t) * k, &w.item0, sizeof(int64_t));
        memcpy(stage.data() + t_fin0 + sizeof(int32_t) * k, &w.fin0, sizeof(int32_t));
    }
    for (const RiskBatchRound &rd : rounds)
        if (rd.items > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld items", (long long)rd.items);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(stage.size()), o_part = lay.take(scratch), o_col = lay.take(sizeof(double) * col_doubles);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out), o_occ = lay.take(sizeof(double) * rows_out);
    const size_t o_out = lay.take(sizeof(double) * 7 * rows_out), o_rresp = lay.take(sizeof(double) * rows_out);
    const size_t o_rtot = lay.take(sizeof(double) * rows_out), o_best = lay.take(2 * sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(lay.size()));
    FX_TRY(r->ev.ensure());
    char *base = r->block;
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    std::vector<RiskWalkArgs> walk(A);
    for (size_t i = 0; i < A; i++) {   // the per-agent argument blocks: the cost kernel's and the re-sum's
        RiskPass &p = q[i];
        const Parts &t = at[i];
        const size_t s0 = o_stage;
        walk[i] = RiskWalkArgs{p.planes, p.ld, p.S, p.n, nullptr, p.flags, D(s0 + t.rec), D(s0 + t.obs), D(s0 + t.pos), D(s0 + t.yaw),
                               D(s0 + t.v), p.K, p.P};
        p.base = base;
        p.o_col = o_col + sizeof(double) * t.col_at, p.o_out = o_out + sizeof(double) * 7 * t.out_at;
        p.o_ids = p.o_bh = s0, p.o_resp = s0 + t.resp;
        p.o_eobs = s0 + t.eobs, p.o_eoff = s0 + t.eoff, p.o_pst = s0 + t.pst, p.o_voff = s0 + t.voff, p.o_vert = s0 + t.vert;
        RiskCostArgs ca{};
        risk_cost_fill(p, &cost[i], ca);
        RespSumArgs &rs = sums[i];
        rs.ids = nullptr;
        rs.resp = D(p.o_out) + 4 * (size_t)p.n;
        rs.pred = t.has_pred ? D(s0 + t.pred) : nullptr;
        rs.resp_out = D(o_rresp) + t.out_at, rs.total = D(o_rtot) + t.out_at;
        memcpy(stage.data() + t_cost + sizeof(RiskCostArgs) * i, &ca, sizeof(ca));
        memcpy(stage.data() + t_sum + sizeof(RespSumArgs) * i, &rs, sizeof(rs));
    }
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const Parts &t = at[g.agent];
        RiskBatchRow w;
        memcpy(&w, stage.data() + t_rows + sizeof(RiskBatchRow) * k, sizeof(w));
        w.w = walk[g.agent];
        w.it.params = reinterpret_cast<const FxRiskParams *>(base + o_stage + t.prm);
        w.it.part = reinterpret_cast<double *>(base + o_part + g.scratch_off);
        w.ego = D(o_ego) + t.out_at, w.obst = D(o_obst) + t.out_at, w.occ = D(o_occ) + t.out_at;
        w.col = D(o_col) + t.col_at;
        memcpy(stage.data() + t_rows + sizeof(RiskBatchRow) * k, &w, sizeof(w));
    }
    HIP_TRY(hipMemcpyAsync(base + o_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream));
    RiskBatchArgs t{};
    t.rows = reinterpret_cast<const RiskBatchRow *>(base + o_stage + t_rows);
    t.item0 = reinterpret_cast<const int64_t *>(base + o_stage + t_item0);
    t.fin0 = reinterpret_cast<const int32_t *>(base + o_stage + t_fin0);
    t.cost = reinterpret_cast<const RiskCostArgs *>(base + o_stage + t_cost);
    t.sum = reinterpret_cast<const RespSumArgs *>(base + o_stage + t_sum);
    t.blk0 = reinterpret_cast<const int32_t *>(base + o_stage + t_blk0);
    t.n_agents = n_agents, t.blocks = (int32_t)blocks;
    long long *d_best = reinterpret_cast<long long *>(base + o_best);
    HIP_TRY(fx_launch_risk_batch(&t, rounds.data(), n_rounds, d_best, r->ev.e0, r->ev.e1, c->stream));
    if (rows_out) {
        const size_t bytes = sizeof(double) * rows_out;
        HIP_TRY(hipMemcpyAsync(out->resp, base + o_rresp, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->total, base + o_rtot, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->ego_risk, base + o_ego, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->obst_risk, base + o_obst, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<long long> best(2 * A);
    HIP_TRY(hipMemcpyAsync(best.data(), d_best, sizeof(long long) * 2 * A, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->ev.e0, r->ev.e1));
    for (size_t i = 0; i < A; i++) {
        out->best_index[i] = (int64_t)best[2 * i];
        memcpy(out->best_cost + i, &best[2 * i + 1], sizeof(double));
    }
    return FX_OK;
}

// The plain risk pass -- fx_eval_risk_agent -- of several agents in ONE call, each with its own id list or none (fxplan.h; DESIGN.md
// section 20).  Per agent the checks of the per-agent entry (risk_check: it resolves planes, ld, flags and the positions of listed
// candidates in a sparse set) and its records; then everything the kernels read -- FxRiskParams, records, obstacle tables, id lists
// (or sparse positions), rows and compact arrays -- in ONE staging buffer and one copy; the rounds of fx_item_rounds over one scratch
// with each row's steps per chunk chosen from its agent's OWN list length, as the per-agent call chooses them.  Runtime calls of a
// call with R rounds: 1 drain (a synchronisation), 1 ensure of the block, 1 copy up, 2 event records, 2 R + 1 launches, 3 copies
// down (ego_risk, obst_risk, min_risk_index), 1 synchronisation -- none of them per agent.
extern "C" int32_t fx_eval_risk_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params, const int64_t *n_ids,
                                      const int64_t *const *ids, const FxRiskBatchOutputs *out) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!params || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "params or out is NULL");
    if (!out->ego_risk || !out->obst_risk || !out->min_risk_index) return set_err(FX_ERR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    if (!fx_launch_risk_list_batch) return set_err(FX_ERR_HIP, "built without the batched risk launcher");
    const int32_t agent0 = agents ? agents[0] : 0;
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "agent %d: no evaluated plan step", agent0);
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d of %d uploaded agents", n_agents, c->n_agents);
    // (the batch is made behind a plan step of all its agents: inputs rewritten since belong to a step that has not run)
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "agent %d: the inputs were rewritten since the last evaluation (fx_update_state): evaluate first", agent0);
    const size_t A = (size_t)n_agents;
    std::vector<RiskPass> q(A);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (size_t i = 0; i < A; i++) {
        const int32_t agent = agents ? agents[i] : (int32_t)i;
        if (agent >= 0 && agent < c->n_agents && listed[agent]) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        const int64_t n_i = n_ids ? n_ids[i] : 0;
        const int64_t *ids_i = (n_ids && ids) ? ids[i] : nullptr;
        if (const int rc = risk_check(q[i], c, agent, params + i, n_i, ids_i, true, false)) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return set_err(rc, "agent %d: %s", agent, why);
        }
        listed[agent] = 1;
    }
    // ONE staging buffer, every part 16-byte aligned; the device's copy lies at o_stage of the block
    std::vector<char> stage;
    auto room = [&](size_t bytes) { const size_t o = stage.size(); stage.resize(o + align_up(std::max<size_t>(bytes, 8), 16), 0); return o; };
    auto put = [&](const void *src, size_t bytes) { const size_t o = room(bytes); if (bytes) memcpy(stage.data() + o, src, bytes); return o; };
    struct Parts { size_t prm, rec, obs, pos, yaw, v, ids, out_at; bool items; };
    std::vector<Parts> at(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<int32_t> cs(A), chunks(A);
    std::vector<double> rec;
    size_t rows_out = 0;
    for (size_t i = 0; i < A; i++) {
        const RiskPass &p = q[i];
        const FxRiskAgent &a = *p.a;
        Parts &t = at[i];
        t = Parts{};
        t.out_at = rows_out;
        rows_out += (size_t)p.n;
        t.prm = put(p.prm, sizeof(FxRiskParams));
        if (p.K > 0) {
            build_records(a, p.S, p.maha, rec);
            t.rec = put(rec.data(), sizeof(double) * rec.size()), t.obs = put(a.obs.data(), sizeof(double) * a.obs.size());
            t.pos = put(a.pos.data(), sizeof(double) * a.pos.size()), t.yaw = put(a.yaw.data(), sizeof(double) * a.yaw.size());
            t.v = put(a.v.data(), sizeof(double) * a.v.size());
        }
        if (p.ids) t.ids = put(p.sparse ? p.pos.data() : p.ids, sizeof(int64_t) * (size_t)p.n);
        // steps per chunk from the agent's OWN list length: what fx_eval_risk_agent chooses for it
        t.items = p.K > 0 && p.S > 1;
        cs[i] = fx_risk_items_chunk_steps(p.n, p.S, p.K);
        chunks[i] = (std::max(p.S - 1, 1) + cs[i] - 1) / cs[i];
        ia[i] = FxItemAgent{p.n, t.items ? sizeof(double) * 2 * (size_t)std::max(p.K, 1) * (size_t)chunks[i] : 0};
    }
    const unsigned long long forced = fx_risk_batch_scratch_forced.load(std::memory_order_relaxed);
    const std::vector<FxItemSegment> segs = fx_item_rounds(ia.data(), n_agents, forced ? (size_t)forced : FX_ITEM_SCRATCH_BYTES);
    const size_t R = segs.size();
    const int n_rounds = R ? segs.back().round + 1 : 0;
    std::vector<RiskBatchRound> rounds((size_t)n_rounds, RiskBatchRound{0, 0, 0, 0});
    std::vector<RiskBatchRow> rows(R);
    std::vector<int32_t> agent_row(A, -1);
    const size_t t_rows = room(sizeof(RiskBatchRow) * R), t_item0 = room(sizeof(int64_t) * R), t_fin0 = room(sizeof(int32_t) * R),
                 t_arow = room(sizeof(int32_t) * A);
    size_t scratch = 0;
    for (size_t k = 0; k < R; k++) {   // the rows' counts (their pointers follow when the block is there)
        const FxItemSegment &g = segs[k];
        const size_t tiles = (size_t)(g.count + 63) / 64;
        RiskBatchRound &rd = rounds[g.round];
        RiskBatchRow &w = rows[k];
        w = RiskBatchRow{};
        if (rd.n_rows == 0) rd.row0 = (int32_t)k;
        rd.n_rows++;
        w.first = g.first, w.count = g.count;
        w.it.nb = (int64_t)tiles * 64, w.it.cs = cs[g.agent], w.it.chunks = chunks[g.agent];
        w.it.need = FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED;
        w.items = at[g.agent].items ? 1 : 0;
        w.item0 = rd.items;
        w.fin0 = rd.fin_blocks;
        if (w.items) rd.items += (int64_t)tiles * chunks[g.agent] * (int64_t)q[g.agent].K;
        const int64_t fin = (int64_t)rd.fin_blocks + (g.count + 255) / 256;
        if (fin > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld workgroups of candidates", (long long)fin);
        rd.fin_blocks = (int32_t)fin;
        scratch = std::max(scratch, g.scratch_off + tiles * 64 * ia[g.agent].per_candidate_bytes);
        agent_row[g.agent] = (int32_t)k;
    }
    for (const RiskBatchRound &rd : rounds)
        if (rd.items > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld items", (long long)rd.items);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(stage.size()), o_part = lay.take(scratch);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out);
    const size_t o_idx = lay.take(sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(lay.size()));
    FX_TRY(r->ev.ensure());
    char *base = r->block;
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const RiskPass &p = q[g.agent];
        const Parts &t = at[g.agent];
        const size_t s0 = o_stage;
        RiskBatchRow &w = rows[k];
        w.w = RiskWalkArgs{p.planes, p.ld, p.S, p.n, p.ids ? reinterpret_cast<const int64_t *>(base + s0 + t.ids) : nullptr, p.flags,
                           D(s0 + t.rec), D(s0 + t.obs), D(s0 + t.pos), D(s0 + t.yaw), D(s0 + t.v), p.K, p.P};
        w.it.params = reinterpret_cast<const FxRiskParams *>(base + s0 + t.prm);
        w.it.part = reinterpret_cast<double *>(base + o_part + g.scratch_off);
        w.ego = D(o_ego) + t.out_at, w.obst = D(o_obst) + t.out_at;
        memcpy(stage.data() + t_item0 + sizeof(int64_t) * k, &w.item0, sizeof(int64_t));
        memcpy(stage.data() + t_fin0 + sizeof(int32_t) * k, &w.fin0, sizeof(int32_t));
    }
    if (R) memcpy(stage.data() + t_rows, rows.data(), sizeof(RiskBatchRow) * R);
    memcpy(stage.data() + t_arow, agent_row.data(), sizeof(int32_t) * A);
    HIP_TRY(hipMemcpyAsync(base + o_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream));
    RiskListBatchArgs t{};
    t.rows = reinterpret_cast<const RiskBatchRow *>(base + o_stage + t_rows);
    t.item0 = reinterpret_cast<const int64_t *>(base + o_stage + t_item0);
    t.fin0 = reinterpret_cast<const int32_t *>(base + o_stage + t_fin0);
    t.agent_row = reinterpret_cast<const int32_t *>(base + o_stage + t_arow);
    t.n_agents = n_agents;
    long long *d_idx = reinterpret_cast<long long *>(base + o_idx);
    HIP_TRY(fx_launch_risk_list_batch(&t, rounds.data(), n_rounds, d_idx, r->ev.e0, r->ev.e1, c->stream));
    if (rows_out) {
        HIP_TRY(hipMemcpyAsync(out->ego_risk, base + o_ego, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->obst_risk, base + o_obst, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<long long> idx(A, -1);
    HIP_TRY(hipMemcpyAsync(idx.data(), d_idx, sizeof(long long) * A, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->ev.e0, r->ev.e1));
    for (size_t i = 0; i < A; i++) {
        // (sparse set: the arg-min ran over positions, which grow with the candidate index -- the same winner, the same tie rule)
        if (q[i].sparse && idx[i] >= 0) idx[i] = (long long)q[i].set.ids[idx[i]];
        out->min_risk_index[i] = (int64_t)idx[i];
    }
    return FX_OK;
}

// The detail and cost passes -- fx_eval_risk_costs_agent -- of several agents in ONE call, each with its own id list or none and
// its own cost parameters or none (fxplan.h).  Per agent the checks of the per-agent entry (risk_check with
// the detail flag, risk_cost_check) and its records; then everything the kernels read -- FxRiskParams, records, obstacle tables, id
// lists (or sparse positions), boundary-harm arrays, responsibility vectors, reach-set tables, rows, compact arrays and the cost
// kernel's argument blocks (risk_cost_fill) -- in ONE staging buffer and one copy; the rounds of fx_item_rounds over one scratch
// with each row's steps per chunk chosen from its agent's OWN list length.  The columns and the principles lie per agent as the
// per-agent kernels' functions index them ([4][K][n] and [7][n]); the caller's are concatenated per column, so a last launch lays
// the column blocks out that way on the device, and the small principle block is laid out on the host.  Runtime calls of a call
// with R rounds: 1 drain (a synchronisation), 1 ensure of the block, 1 copy up, 2 event records, 2 R + 4 launches (2 R + 1 where no
// agent has cost parameters and no column is asked for), at most 9 copies down (ego_risk, obst_risk, obst_harm_occ, the four
// columns, the principle block, the two arg-mins), 1 synchronisation -- none of them per agent.
extern "C" int32_t fx_eval_risk_costs_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params,
                                            const FxRiskCostParams *const *cost, const int64_t *n_ids, const int64_t *const *ids,
                                            const FxRiskCostBatchOutputs *out) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!params || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "params or out is NULL");
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    if (!fx_launch_risk_costs_batch) return set_err(FX_ERR_HIP, "built without the batched risk-cost launcher");
    const int32_t agent0 = agents ? agents[0] : 0;
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "agent %d: no evaluated plan step", agent0);
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d of %d uploaded agents", n_agents, c->n_agents);
    // (the batch is made behind a plan step of all its agents: inputs rewritten since belong to a step that has not run)
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "agent %d: the inputs were rewritten since the last evaluation (fx_update_state): evaluate first", agent0);
    const size_t A = (size_t)n_agents;
    std::vector<RiskPass> q(A);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (size_t i = 0; i < A; i++) {
        const int32_t agent = agents ? agents[i] : (int32_t)i;
        if (agent >= 0 && agent < c->n_agents && listed[agent]) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        const int64_t n_i = n_ids ? n_ids[i] : 0;
        const int64_t *ids_i = (n_ids && ids) ? ids[i] : nullptr;
        int rc = risk_check(q[i], c, agent, params + i, n_i, ids_i, true, true);
        if (!rc && cost && cost[i]) rc = risk_cost_check(q[i], cost[i]);
        if (rc) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return set_err(rc, "agent %d: %s", agent, why);
        }
        listed[agent] = 1;
    }
    // ONE staging buffer, every part 16-byte aligned; the device's copy lies at o_stage of the block
    std::vector<char> stage;
    auto room = [&](size_t bytes) { const size_t o = stage.size(); stage.resize(o + align_up(std::max<size_t>(bytes, 8), 16), 0); return o; };
    auto put = [&](const void *src, size_t bytes) { const size_t o = room(bytes); if (bytes) memcpy(stage.data() + o, src, bytes); return o; };
    struct Parts { size_t prm, rec, obs, pos, yaw, v, ids, bh, resp, eobs, eoff, pst, voff, vert, out_at, col_at, cout_at; int ci; bool items; };
    std::vector<Parts> at(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<int32_t> cs(A), chunks(A), blk0;
    std::vector<double> rec;
    size_t rows_out = 0, col_doubles = 0, rows_cost = 0;
    int64_t blocks = 0;
    for (size_t i = 0; i < A; i++) {
        RiskPass &p = q[i];
        const FxRiskAgent &a = *p.a;
        const FxRiskCostParams *cp = cost ? cost[i] : nullptr;
        Parts &t = at[i];
        t = Parts{};
        t.out_at = rows_out, t.col_at = col_doubles, t.cout_at = rows_cost, t.ci = -1;
        rows_out += (size_t)p.n;
        col_doubles += 4 * (size_t)p.K * (size_t)p.n;
        t.prm = put(p.prm, sizeof(FxRiskParams));
        if (p.K > 0) {
            build_records(a, p.S, p.maha, rec);
            t.rec = put(rec.data(), sizeof(double) * rec.size()), t.obs = put(a.obs.data(), sizeof(double) * a.obs.size());
            t.pos = put(a.pos.data(), sizeof(double) * a.pos.size()), t.yaw = put(a.yaw.data(), sizeof(double) * a.yaw.size());
            t.v = put(a.v.data(), sizeof(double) * a.v.size());
        }
        if (p.ids) t.ids = put(p.sparse ? p.pos.data() : p.ids, sizeof(int64_t) * (size_t)p.n);
        if (cp) {   // (what risk_stage and risk_cost_args take and upload for a cost pass)
            t.ci = (int)blk0.size();
            blk0.push_back((int32_t)blocks);
            blocks += (p.n + 255) / 256;
            rows_cost += (size_t)p.n;
            if (cp->boundary_mode == FX_RISK_BOUNDARY_ARRAY) t.bh = put(cp->boundary_harm, sizeof(double) * (size_t)p.n);
            if (cp->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && p.K > 0) t.resp = put(cp->responsibility, sizeof(double) * p.K);
            if (cp->responsibility_mode == FX_RISK_RESP_REACH_SET) {
                p.nE = a.rs_obs.size(), p.nP = a.rs_step.size(), p.nV = a.rs_verts.size() / 2;
                t.eobs = put(a.rs_obs.data(), sizeof(int32_t) * p.nE), t.eoff = put(a.rs_off.data(), sizeof(int32_t) * a.rs_off.size());
                t.pst = put(a.rs_step.data(), sizeof(int32_t) * p.nP), t.voff = put(a.rs_voff.data(), sizeof(int32_t) * a.rs_voff.size());
                t.vert = put(a.rs_verts.data(), sizeof(double) * a.rs_verts.size());
            }
        }
        // steps per chunk from the agent's OWN list length: what fx_eval_risk_costs_agent chooses for it
        t.items = p.K > 0 && p.S > 1;
        cs[i] = fx_risk_items_chunk_steps(p.n, p.S, p.K);
        chunks[i] = (std::max(p.S - 1, 1) + cs[i] - 1) / cs[i];
        ia[i] = FxItemAgent{p.n, t.items ? sizeof(double) * 7 * (size_t)p.K * (size_t)chunks[i] : 0};
    }
    const size_t NC = blk0.size();
    if (blocks > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "%lld workgroups of candidates", (long long)blocks);
    // the caller's columns are concatenated per column: where one is asked for, a last launch lays the agents' [4][K][n] blocks out
    // that way on the device (RiskCopySeg: one plane of one agent, 1 024 doubles per workgroup), and each column comes down in one copy
    double *const cols[4] = {out->ego_risk_max, out->obst_risk_max, out->ego_harm_max, out->obst_harm_max};
    const bool any_col = (cols[0] || cols[1] || cols[2] || cols[3]) && col_doubles > 0;
    const size_t NS = any_col ? 4 * A : 0, T = col_doubles / 4;
    std::vector<int32_t> seg_blk0(NS);
    int64_t seg_blocks = 0;
    for (size_t k = 0; k < NS; k++) {
        seg_blk0[k] = (int32_t)seg_blocks;
        seg_blocks += ((int64_t)q[k / 4].K * q[k / 4].n + 1023) / 1024;
        if (seg_blocks > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "%lld workgroups of column values", (long long)seg_blocks);
    }
    const unsigned long long forced = fx_risk_batch_scratch_forced.load(std::memory_order_relaxed);
    const std::vector<FxItemSegment> segs = fx_item_rounds(ia.data(), n_agents, forced ? (size_t)forced : FX_ITEM_SCRATCH_BYTES);
    const size_t R = segs.size();
    const int n_rounds = R ? segs.back().round + 1 : 0;
    std::vector<RiskBatchRound> rounds((size_t)n_rounds, RiskBatchRound{0, 0, 0, 0});
    std::vector<RiskBatchRow> rows(R);
    std::vector<int32_t> agent_row(A, -1);
    const size_t t_rows = room(sizeof(RiskBatchRow) * R), t_item0 = room(sizeof(int64_t) * R), t_fin0 = room(sizeof(int32_t) * R),
                 t_arow = room(sizeof(int32_t) * A), t_cost = room(sizeof(RiskCostArgs) * NC), t_blk0 = put(blk0.data(), sizeof(int32_t) * NC),
                 t_seg = room(sizeof(RiskCopySeg) * NS), t_sblk = put(seg_blk0.data(), sizeof(int32_t) * NS);
    size_t scratch = 0;
    for (size_t k = 0; k < R; k++) {   // the rows' counts (their pointers follow when the block is there)
        const FxItemSegment &g = segs[k];
        const size_t tiles = (size_t)(g.count + 63) / 64;
        RiskBatchRound &rd = rounds[g.round];
        RiskBatchRow &w = rows[k];
        w = RiskBatchRow{};
        if (rd.n_rows == 0) rd.row0 = (int32_t)k;
        rd.n_rows++;
        w.first = g.first, w.count = g.count;
        w.it.nb = (int64_t)tiles * 64, w.it.cs = cs[g.agent], w.it.chunks = chunks[g.agent];
        w.it.need = FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED;
        w.items = at[g.agent].items ? 1 : 0;
        w.item0 = rd.items;
        w.fin0 = rd.fin_blocks;
        if (w.items) rd.items += (int64_t)tiles * chunks[g.agent] * (int64_t)q[g.agent].K;
        const int64_t fin = (int64_t)rd.fin_blocks + (g.count + 255) / 256;
        if (fin > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld workgroups of candidates", (long long)fin);
        rd.fin_blocks = (int32_t)fin;
        scratch = std::max(scratch, g.scratch_off + tiles * 64 * ia[g.agent].per_candidate_bytes);
        agent_row[g.agent] = (int32_t)k;
    }
    for (const RiskBatchRound &rd : rounds)
        if (rd.items > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld items", (long long)rd.items);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(stage.size()), o_part = lay.take(scratch), o_col = lay.take(sizeof(double) * col_doubles);
    const size_t o_cat = lay.take(any_col ? sizeof(double) * col_doubles : 0);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out), o_occ = lay.take(sizeof(double) * rows_out);
    const size_t o_out = lay.take(sizeof(double) * 7 * rows_cost), o_idx = lay.take(sizeof(long long) * (A + NC));
    FxRiskState *r = q[0].r;
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(lay.size()));
    FX_TRY(r->ev.ensure());
    char *base = r->block;
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    const size_t s0 = o_stage;
    for (size_t i = 0; i < A; i++) {   // the cost kernel's argument blocks, from where the agent's parts lie
        const Parts &t = at[i];
        if (t.ci < 0) continue;
        RiskPass &p = q[i];
        p.base = base;
        p.o_col = o_col + sizeof(double) * t.col_at, p.o_out = o_out + sizeof(double) * 7 * t.cout_at;
        p.o_ids = s0 + t.ids, p.o_bh = s0 + t.bh, p.o_resp = s0 + t.resp;
        p.o_eobs = s0 + t.eobs, p.o_eoff = s0 + t.eoff, p.o_pst = s0 + t.pst, p.o_voff = s0 + t.voff, p.o_vert = s0 + t.vert;
        RiskCostArgs ca{};
        risk_cost_fill(p, cost[i], ca);
        memcpy(stage.data() + t_cost + sizeof(RiskCostArgs) * (size_t)t.ci, &ca, sizeof(ca));
    }
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const RiskPass &p = q[g.agent];
        const Parts &t = at[g.agent];
        RiskBatchRow &w = rows[k];
        w.w = RiskWalkArgs{p.planes, p.ld, p.S, p.n, p.ids ? reinterpret_cast<const int64_t *>(base + s0 + t.ids) : nullptr, p.flags,
                           D(s0 + t.rec), D(s0 + t.obs), D(s0 + t.pos), D(s0 + t.yaw), D(s0 + t.v), p.K, p.P};
        w.it.params = reinterpret_cast<const FxRiskParams *>(base + s0 + t.prm);
        w.it.part = reinterpret_cast<double *>(base + o_part + g.scratch_off);
        w.ego = D(o_ego) + t.out_at, w.obst = D(o_obst) + t.out_at, w.occ = D(o_occ) + t.out_at;
        w.col = D(o_col) + t.col_at;
        memcpy(stage.data() + t_item0 + sizeof(int64_t) * k, &w.item0, sizeof(int64_t));
        memcpy(stage.data() + t_fin0 + sizeof(int32_t) * k, &w.fin0, sizeof(int32_t));
    }
    if (R) memcpy(stage.data() + t_rows, rows.data(), sizeof(RiskBatchRow) * R);
    memcpy(stage.data() + t_arow, agent_row.data(), sizeof(int32_t) * A);
    for (size_t k = 0; k < NS; k++) {   // plane k % 4 of agent k / 4: from its block to its place in that column of the call
        const Parts &pt = at[k / 4];
        const size_t Kn = (size_t)q[k / 4].K * (size_t)q[k / 4].n;
        const RiskCopySeg g{D(o_col) + pt.col_at + (k % 4) * Kn, D(o_cat) + (k % 4) * T + pt.col_at / 4, (int64_t)Kn};
        memcpy(stage.data() + t_seg + sizeof(RiskCopySeg) * k, &g, sizeof(g));
    }
    HIP_TRY(hipMemcpyAsync(base + o_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream));
    RiskCostBatchArgs t{};
    t.rows = reinterpret_cast<const RiskBatchRow *>(base + o_stage + t_rows);
    t.item0 = reinterpret_cast<const int64_t *>(base + o_stage + t_item0);
    t.fin0 = reinterpret_cast<const int32_t *>(base + o_stage + t_fin0);
    t.agent_row = reinterpret_cast<const int32_t *>(base + o_stage + t_arow);
    t.cost = reinterpret_cast<const RiskCostArgs *>(base + o_stage + t_cost);
    t.blk0 = reinterpret_cast<const int32_t *>(base + o_stage + t_blk0);
    t.n_agents = n_agents, t.n_cost = (int32_t)NC, t.blocks = (int32_t)blocks;
    t.seg = reinterpret_cast<const RiskCopySeg *>(base + o_stage + t_seg);
    t.seg_blk0 = reinterpret_cast<const int32_t *>(base + o_stage + t_sblk);
    t.n_seg = (int32_t)NS, t.seg_blocks = (int32_t)seg_blocks;
    long long *d_idx = reinterpret_cast<long long *>(base + o_idx);
    HIP_TRY(fx_launch_risk_costs_batch(&t, rounds.data(), n_rounds, d_idx, d_idx + A, r->ev.e0, r->ev.e1, c->stream));
    auto down = [&](double *dst, size_t o, size_t count) {
        return (dst && count) ? hipMemcpyAsync(dst, base + o, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIP_TRY(down(out->ego_risk, o_ego, rows_out));
    HIP_TRY(down(out->obst_risk, o_obst, rows_out));
    HIP_TRY(down(out->obst_harm_occ, o_occ, rows_out));
    if (any_col)
        for (int k = 0; k < 4; k++) HIP_TRY(down(cols[k], o_cat + sizeof(double) * k * T, T));
    // the principles: an agent without cost parameters has rows in the caller's arrays that stay unwritten, so the (small) block
    // [7][n] per agent comes down into memory of the call and is laid out from there (uninitialised: every double read below has
    // been written by a kernel and copied)
    double *const pr[7] = {out->bayes, out->equality, out->maximin, out->ego, out->responsibility, out->total, out->boundary_harm};
    bool any_pr = false;
    for (double *x : pr) any_pr = any_pr || x;
    const size_t n_out = any_pr ? 7 * rows_cost : 0;
    const std::unique_ptr<double[]> h_out(n_out ? new double[n_out] : nullptr);
    HIP_TRY(down(h_out.get(), o_out, n_out));
    std::vector<long long> idx(A + NC, -1);
    HIP_TRY(hipMemcpyAsync(idx.data(), d_idx, sizeof(long long) * (A + NC), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->ev.e0, r->ev.e1));
    r->last_rounds = n_rounds;
    for (size_t i = 0; i < A; i++) {
        const Parts &pt = at[i];
        const size_t nn = (size_t)q[i].n;
        if (pt.ci >= 0 && h_out)
            for (int k = 0; k < 7; k++)
                if (pr[k] && nn) memcpy(pr[k] + pt.out_at, h_out.get() + 7 * pt.cout_at + k * nn, sizeof(double) * nn);
        // (sparse set: the arg-mins ran over positions, which grow with the candidate index -- the same winner, the same tie rule)
        long long ri = idx[i], ci = pt.ci >= 0 ? idx[A + (size_t)pt.ci] : -1;
        if (q[i].sparse && ri >= 0) ri = (long long)q[i].set.ids[ri];
        if (q[i].sparse && ci >= 0) ci = (long long)q[i].set.ids[ci];
        if (out->min_risk_index) out->min_risk_index[i] = (int64_t)ri;
        if (out->min_cost_index) out->min_cost_index[i] = (int64_t)ci;
    }
    return FX_OK;
}

// (hook of the tests, not part of fxplan.h: the rounds of scratch the last fx_eval_risk_costs_batch call took; -1 before the first)
extern "C" int32_t fx_last_risk_costs_batch_rounds(FxContext *c) { return (c && c->risk) ? c->risk->last_rounds : -1; }

extern "C" double fx_last_predprob_ms(FxContext *c) { return (c && c->risk) ? (double)c->risk->last_pp_ms : -1.0; }

extern "C" double fx_last_risk_ms(FxContext *c) { return (c && c->risk) ? (double)c->risk->last_ms : -1.0; }
