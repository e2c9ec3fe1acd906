// fx_api_risk.hip -- C-ABI of the trajectory risk (fx_risk_kernel.h): the obstacle tables of an agent and
// the risk pass with its arg-min over the materialised bundle of the last plan step (or, for listed candidates of a step that stored
// none, over the agent's sparse set: fx_api_materialise.hip); the reach sets of an agent and the detail /
// risk-cost pass.  The two evaluations share one host path (RiskPass) and one device block.  Nothing of
// this runs in a plan step.  The collision probability as the prediction cost (fx_predprob_kernel.h) is a third
// entrance on the same host path: the same checks, records, uploads and block; fx_eval_prediction_prob_batch
// is that pass for several agents in one call: the same checks and records per agent, one staging buffer for records and tables;
// fx_eval_responsibility_cost_batch is the responsibility pass for several agents in one call, and
// fx_eval_risk_batch the plain risk pass for several agents, each with an id list or none, and
// fx_eval_risk_costs_batch the detail and cost passes for several agents, with lists and cost parameters each.
#include <atomic>
#include <cmath>
#include <memory>
#include <vector>

#include "fx_pass.h"
#include "fx_rescore_batch_plan.h"   // fx_resp_term_at: where the responsibility term stands in a cost list
#include "fx_risk_args.h"

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
// The same for the prediction-probability items: what fx_launch_predprob (fx_kernels.hip) and the batched pass below size their
// chunks by, or what fx_predprob_set_chunk_steps forces (tests: the results do not depend on it)
static std::atomic<int> fx_predprob_chunk_forced{0};
extern "C" void fx_predprob_set_chunk_steps(int32_t steps) { fx_predprob_chunk_forced.store(steps > 0 ? steps : 0, std::memory_order_relaxed); }
extern "C" int32_t fx_predprob_chunk_steps(int64_t n, int32_t S, int32_t K) {
    return fx_item_chunk_steps(n, S, K, fx_predprob_chunk_forced.load(std::memory_order_relaxed));
}

// What every pass does before it touches the device: the stream drained, the passes' one block at `bytes` or more, the events
static int risk_block(FxContext *c, FxRiskState *r, size_t bytes, char *&base) {
    HIP_TRY(hipSetDevice(c->device));
    FX_TRY(fx_drain(c));
    FX_TRY(r->block.ensure(bytes));
    FX_TRY(r->ev.ensure());
    base = r->block;
    return FX_OK;
}

// The end of every pass: its n arg-min words come down behind its outputs, the ONE synchronisation, the device time into *ms
static int risk_end(FxContext *c, FxRiskState *r, const void *d_idx, long long *idx, size_t n, float *ms) {
    HIP_TRY(hipMemcpyAsync(idx, d_idx, sizeof(long long) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(ms, r->ev.e0, r->ev.e1));
    return FX_OK;
}
// ... and the candidate an arg-min names: over a sparse set it ran over positions, which grow with the candidate index -- the
// same winner, the same tie rule
static int64_t risk_winner(const RiskPass &q, long long i) { return (q.sparse && i >= 0) ? q.set.ids[i] : (int64_t)i; }

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
    FX_TRY(risk_block(c, r, lay.size(), q.base));
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
    FX_TRY(risk_end(c, r, d_idx, idx, ca ? 2 : 1, &r->last_ms));
    if (out.min_risk_index) *out.min_risk_index = risk_winner(q, idx[0]);
    if (out.min_cost_index) *out.min_cost_index = risk_winner(q, idx[1]);
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

// where the parts of a cost pass lie on the device: the per-agent pass has them in its block (risk_stage), a batched call in its
// staging buffer and its outputs
struct RiskCostPtrs {
    const double *col;         // [4][K][n] of the detail pass
    const int64_t *ids;        // the list the walk got, or null
    const double *bh, *resp;   // the caller's boundary harm [n] and responsibility vector [K]
    const int32_t *eobs, *eoff, *pst, *voff;   // the reach-set tables
    const double *vert;
    double *out;               // [7][n]
};

// the argument block of a cost pass's kernel from what risk_check established of the agent and where the parts lie: no HIP call
static void risk_cost_fill(const RiskPass &q, const FxRiskCostParams *cost, const RiskCostPtrs &d, RiskCostArgs &ca) {
    ca.col = d.col;
    ca.n = q.n;
    ca.ids = d.ids;
    ca.flags = q.flags;
    ca.planes = q.planes;
    ca.ld = q.ld;
    ca.S = q.S;
    ca.K = q.K;
    ca.bh_in = cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY ? d.bh : nullptr;
    ca.bstep = (cost->boundary_mode == FX_RISK_BOUNDARY_STEP && (q.s->mode & FX_MODE_ROAD_BOUNDARY)) ? q.bstep : nullptr;
    ca.bh_c = cost->boundary_c;
    ca.bh_s = cost->boundary_s;
    ca.resp_mode = cost->responsibility_mode;
    ca.n_entries = (int32_t)q.nE;
    ca.resp = d.resp;
    ca.entry_obs = d.eobs;
    ca.entry_off = d.eoff;
    ca.part_step = d.pst;
    ca.vert_off = d.voff;
    ca.verts = d.vert;
    for (int k = 0; k < 5; k++) ca.w[k] = cost->weights[k];
    ca.eps = cost->maximin_eps;
    ca.scale = cost->maximin_scale;
    ca.out = d.out;
}

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
    risk_cost_fill(q, cost, RiskCostPtrs{q.D(q.o_col), q.d_ids(), q.D(q.o_bh), q.D(q.o_resp), q.I(q.o_eobs), q.I(q.o_eoff), q.I(q.o_pst),
                                         q.I(q.o_voff), q.D(q.o_vert), q.D(q.o_out)}, ca);
    return FX_OK;
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
    FX_TRY(fx_check_inputs_current(c));   // (the condition of fx_eval_prediction_prob_agent: the planes and cost rows are the last evaluated step's)
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
    rs.n_pred = fx_prediction_term(hp);
    rs.at = fx_resp_term_at(hp.cost_id, hp.n_cost);   // in front of the first name behind "responsibility" in the sorted list
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
    *out->best_index = risk_winner(q, best[0]);
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
    FX_TRY(fx_check_inputs_current(c));   // (check_agent has established `evaluated`)
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
    n_pred = fx_prediction_term(c->h_probs[agent]);
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
    FX_TRY(risk_end(c, r, d_best, best, 2, &r->last_pp_ms));
    if (out->best_index) *out->best_index = risk_winner(q, best[0]);
    if (out->best_cost) memcpy(out->best_cost, &best[1], sizeof(double));
    return FX_OK;
}

// ---- Several agents in ONE call (fxplan.h; DESIGN.md sections 18 to 21) ----
// The four entries at the end make the same call, each for its pass, out of these pieces: batch_front (the refusals that need no
// device, then the per-agent entry's own checks agent by agent); RiskStage (ONE staging buffer for everything the kernels read and
// one copy up); risk_put_agent / risk_put_cost (what an agent uploads); risk_item_share (its steps per chunk and scratch share);
// fx_item_rounds and fx_item_table (fx_pass.h: the rounds over one scratch, the rows' and rounds' sizes, the capacity refusals);
// risk_block; risk_fill_rows; risk_cost_fill; risk_end and risk_winner.  None of them makes a runtime call per agent.

// The front of a call: the refusals in the order the entries report them.  missing: what of the call's own arguments is NULL, or
// null; name_agent: the refusal of a context without an evaluated step names the first agent; current: the call needs the inputs of the last evaluation (fx_inputs_current).  check is
// the per-agent entry's check of agent `agent`, the i-th of the call, into q[i]; its refusal is reported as "agent <agent>: ...".
// n_agents == 0 returns FX_OK with nothing touched: the caller returns then too.
template <class Check>
static int batch_front(FxContext *c, const char *missing, int32_t n_agents, const int32_t *agents, bool name_agent, bool current,
                       std::vector<RiskPass> &q, Check check) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (missing) return set_err(FX_ERR_INVALID_ARGUMENT, "%s", missing);
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    const int32_t agent0 = agents ? agents[0] : 0;
    if (!c->evaluated)
        return name_agent ? set_err(FX_ERR_NOT_READY, "agent %d: no evaluated plan step", agent0) : set_err(FX_ERR_NOT_READY, "no evaluated plan step");
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d of %d uploaded agents", n_agents, c->n_agents);
    // (a batch is made behind a plan step of all its agents: inputs rewritten since belong to a step that has not run)
    if (current && !fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "agent %d: the inputs were rewritten since the last evaluation (fx_update_state): evaluate first", agent0);
    q.resize((size_t)n_agents);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (size_t i = 0; i < q.size(); i++) {
        const int32_t agent = agents ? agents[i] : (int32_t)i;
        if (agent >= 0 && agent < c->n_agents && listed[agent]) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        if (const int rc = check(q[i], i, agent)) {
            char why[sizeof(g_err)];
            snprintf(why, sizeof(why), "%s", g_err);
            return set_err(rc, "agent %d: %s", agent, why);
        }
        listed[agent] = 1;   // (the check has refused an agent out of range)
    }
    return FX_OK;
}

// The ONE staging buffer of a call, every part 16-byte aligned and at least 8 bytes; offsets count from its start, and the
// device's copy lies at the start of the block.
struct RiskStage {
    std::vector<char> bytes;
    size_t room(size_t n) { const size_t o = bytes.size(); bytes.resize(o + align_up(std::max<size_t>(n, 8), 16), 0); return o; }
    size_t put(const void *src, size_t n) { const size_t o = room(n); if (n) memcpy(bytes.data() + o, src, n); return o; }
    template <class T> size_t put(const std::vector<T> &v) { return put(v.data(), sizeof(T) * v.size()); }
};

// What every agent of a risk pass uploads (risk_stage, for one agent): its FxRiskParams, records and obstacle tables, and its id
// list or the list's positions in its sparse set.  rec: the records' buffer, reused from agent to agent.
struct RiskAgentAt { size_t prm, rec, obs, pos, yaw, v, ids; };
static RiskAgentAt risk_put_agent(RiskStage &st, const RiskPass &p, std::vector<double> &rec) {
    const FxRiskAgent &a = *p.a;
    RiskAgentAt t{};
    t.prm = st.put(p.prm, sizeof(FxRiskParams));
    if (p.K > 0) {   // (without an obstacle no kernel reads any of these)
        build_records(a, p.S, p.maha, rec);
        t.rec = st.put(rec), t.obs = st.put(a.obs), t.pos = st.put(a.pos), t.yaw = st.put(a.yaw), t.v = st.put(a.v);
    }
    if (p.ids) t.ids = st.put(p.sparse ? p.pos.data() : p.ids, sizeof(int64_t) * (size_t)p.n);
    return t;
}
// ... and what its cost pass uploads on top (risk_stage and risk_cost_args, for one agent): the caller's boundary harm and
// responsibility vector, the reach-set tables; it counts the latter into p
struct RiskCostAt { size_t bh, resp, eobs, eoff, pst, voff, vert; };
static RiskCostAt risk_put_cost(RiskStage &st, RiskPass &p, const FxRiskCostParams *cp) {
    const FxRiskAgent &a = *p.a;
    RiskCostAt t{};
    if (cp->boundary_mode == FX_RISK_BOUNDARY_ARRAY) t.bh = st.put(cp->boundary_harm, sizeof(double) * (size_t)p.n);
    if (cp->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && p.K > 0) t.resp = st.put(cp->responsibility, sizeof(double) * p.K);
    if (cp->responsibility_mode == FX_RISK_RESP_REACH_SET) {
        p.nE = a.rs_obs.size(), p.nP = a.rs_step.size(), p.nV = a.rs_verts.size() / 2;
        t.eobs = st.put(a.rs_obs), t.eoff = st.put(a.rs_off), t.pst = st.put(a.rs_step), t.voff = st.put(a.rs_voff), t.vert = st.put(a.rs_verts);
    }
    return t;
}

// Steps per chunk of an agent's items from its OWN size, as the per-agent entry chooses them, and one candidate's share of the
// scratch -- nv partials per (obstacle, chunk) -- none where the agent runs no item (K = 0 or S = 1)
struct RiskItemShare {
    int32_t cs, chunks;
    int64_t per_tile;   // items per tile of 64 candidates
};
static FxItemAgent risk_item_share(const RiskPass &p, int nv, RiskItemShare &sh) {
    const bool items = p.K > 0 && p.S > 1;
    sh.cs = fx_risk_items_chunk_steps(p.n, p.S, p.K);
    sh.chunks = (std::max(p.S - 1, 1) + sh.cs - 1) / sh.cs;
    sh.per_tile = items ? (int64_t)sh.chunks * p.K : 0;
    return FxItemAgent{p.n, items ? sizeof(double) * (size_t)nv * (size_t)p.K * (size_t)sh.chunks : 0};
}

// an agent of a batched risk pass: where its parts lie in the stage, its items, and its rows of the call's outputs (in doubles)
struct RiskBatchAgent {
    RiskAgentAt at;
    RiskCostAt cost;
    RiskItemShare sh;
    size_t out_at, col_at;   // of [n] per agent; of [4][K][n] per agent
    int ci;                  // its place among the agents with a cost pass, -1 without one
    size_t cout_at;          // of [n] per agent with a cost pass
};

static std::atomic<long long> fx_predprob_scratch_forced{0};
extern "C" void fx_predprob_set_scratch_limit(int64_t bytes) { fx_predprob_scratch_forced.store(bytes > 0 ? bytes : 0, std::memory_order_relaxed); }
static std::atomic<unsigned long long> fx_risk_batch_scratch_forced{0};
extern "C" void fx_risk_batch_set_scratch_limit(size_t bytes) { fx_risk_batch_scratch_forced.store(bytes, std::memory_order_relaxed); }

// the rounds and the table of a batched risk pass from its agents' shares
static int risk_batch_table(const std::vector<FxItemAgent> &ia, const std::vector<RiskBatchAgent> &ag, std::vector<FxItemSegment> &segs,
                            FxItemTable &tab) {
    const unsigned long long forced = fx_risk_batch_scratch_forced.load(std::memory_order_relaxed);
    segs = fx_item_rounds(ia.data(), (int)ia.size(), forced ? (size_t)forced : FX_ITEM_SCRATCH_BYTES);
    std::vector<int64_t> per_tile(segs.size());
    for (size_t k = 0; k < segs.size(); k++) per_tile[k] = ag[segs[k].agent].sh.per_tile;
    return fx_item_table(segs, ia.data(), (int)ia.size(), per_tile.data(), tab);
}

// The device tables of a call in the stage: room for them while the stage is laid out, and -- the block is there, the rows have
// their pointers -- their contents and where the device's copy has them (d_stage: its start)
struct BatchTableAt { size_t rows, item0, fin0, arow; };
template <class Row>
static BatchTableAt batch_table_room(RiskStage &st, size_t R, size_t A) {
    BatchTableAt t;
    t.rows = st.room(sizeof(Row) * R), t.item0 = st.room(sizeof(int64_t) * R), t.fin0 = st.room(sizeof(int32_t) * R);
    t.arow = st.room(sizeof(int32_t) * A);
    return t;
}
template <class Row>
static BatchTable<Row> batch_table_put(RiskStage &st, const BatchTableAt &t, const std::vector<Row> &rows, const FxItemTable &tab,
                                       const char *d_stage) {
    const size_t R = rows.size(), A = tab.agent_row.size();
    if (R) {
        memcpy(st.bytes.data() + t.rows, rows.data(), sizeof(Row) * R);
        memcpy(st.bytes.data() + t.item0, tab.item0.data(), sizeof(int64_t) * R);
        memcpy(st.bytes.data() + t.fin0, tab.fin0.data(), sizeof(int32_t) * R);
    }
    memcpy(st.bytes.data() + t.arow, tab.agent_row.data(), sizeof(int32_t) * A);
    return BatchTable<Row>{reinterpret_cast<const Row *>(d_stage + t.rows), reinterpret_cast<const int64_t *>(d_stage + t.item0),
                           reinterpret_cast<const int32_t *>(d_stage + t.fin0), reinterpret_cast<const int32_t *>(d_stage + t.arow), (int32_t)A};
}

// The rows of a batched risk pass: each segment's counts from the table and its agent's pointers from where the agent's parts lie
// in the device's copy of the stage (d_stage), its segment of the round's scratch (d_part) and its rows of the call's outputs
// (occ, col: null in the plain pass).  need: the flags a candidate of an agent without a list needs.
static std::vector<RiskBatchRow> risk_fill_rows(const std::vector<FxItemSegment> &segs, const FxItemTable &tab, const std::vector<RiskPass> &q,
                                                const std::vector<RiskBatchAgent> &ag, uint32_t need, char *d_stage, char *d_part,
                                                double *ego, double *obst, double *occ, double *col) {
    std::vector<RiskBatchRow> rows(segs.size(), RiskBatchRow{});
    auto D = [&](size_t o) { return reinterpret_cast<double *>(d_stage + o); };
    for (size_t k = 0; k < segs.size(); k++) {
        const FxItemSegment &g = segs[k];
        const RiskPass &p = q[g.agent];
        const RiskBatchAgent &b = ag[g.agent];
        const RiskAgentAt &t = b.at;
        RiskBatchRow &w = rows[k];
        w.w = RiskWalkArgs{p.planes, p.ld, p.S, p.n, p.ids ? reinterpret_cast<const int64_t *>(d_stage + t.ids) : nullptr, p.flags,
                           D(t.rec), D(t.obs), D(t.pos), D(t.yaw), D(t.v), p.K, p.P};
        w.it.params = reinterpret_cast<const FxRiskParams *>(d_stage + t.prm);
        w.it.part = reinterpret_cast<double *>(d_part + g.scratch_off);
        w.it.nb = tab.nb[k], w.it.cs = b.sh.cs, w.it.chunks = b.sh.chunks, w.it.need = need;
        w.first = g.first, w.count = g.count;
        w.item0 = tab.item0[k], w.fin0 = tab.fin0[k], w.items = b.sh.per_tile ? 1 : 0;
        w.ego = ego + b.out_at, w.obst = obst + b.out_at, w.occ = occ ? occ + b.out_at : nullptr;
        w.col = col ? col + b.col_at : nullptr;
    }
    return rows;
}

// where the parts of an agent's cost pass lie in a batched call: in the device's copy of the stage, but for its columns and outputs
static RiskCostPtrs risk_batch_cost_ptrs(const char *d_stage, const RiskPass &p, const RiskBatchAgent &b, const double *col, double *out) {
    auto D = [&](size_t o) { return reinterpret_cast<const double *>(d_stage + o); };
    auto I = [&](size_t o) { return reinterpret_cast<const int32_t *>(d_stage + o); };
    return RiskCostPtrs{col, p.ids ? reinterpret_cast<const int64_t *>(d_stage + b.at.ids) : nullptr, D(b.cost.bh), D(b.cost.resp),
                        I(b.cost.eobs), I(b.cost.eoff), I(b.cost.pst), I(b.cost.voff), D(b.cost.vert), out};
}

// The prediction-probability pass over every candidate of several agents: the checks of
// fx_eval_prediction_prob_agent (predprob_check); the stage holds the records of the agents that run items and the tables; a
// row's steps per chunk come from its ROUND's tiles x obstacles, not from its agent.  Runtime calls of a call with R rounds: 1
// drain (a synchronisation), 1 ensure of the block, 1 copy up, 2 event records, 2 R + 1 launches, 3 copies down (prob, total,
// best), 1 synchronisation.
extern "C" int32_t fx_eval_prediction_prob_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxPredProbParams *params,
                                                 const FxPredProbBatchOutputs *out) {
    std::vector<RiskPass> q;
    std::vector<int> n_pred;   // (sized in the check: the front has accepted n_agents by then)
    const int rc = batch_front(c, (!params || !out) ? "params or out is NULL" : nullptr, n_agents, agents, false, false, q,
                               [&](RiskPass &p, size_t i, int32_t agent) {
        n_pred.resize(q.size());
        return predprob_check(p, c, agent, params + i, 0, nullptr, true, n_pred[i]);
    });
    if (rc || n_agents == 0) return rc;
    const size_t A = (size_t)n_agents;
    // one candidate's share of the scratch: a probability per (obstacle, step), none where no item runs
    RiskStage st;
    std::vector<double> rec;
    std::vector<size_t> rec_at(A, 0), out_at(A);
    std::vector<FxItemAgent> ia(A);
    size_t rows_out = 0;
    for (size_t i = 0; i < A; i++) {
        const RiskPass &p = q[i];
        out_at[i] = rows_out;
        rows_out += (size_t)p.n;
        const bool items = params[i].source == FX_PRED_SOURCE_PROBABILITY && p.K > 0 && p.S > 1;
        if (items) {
            build_records(*p.a, p.S, false, rec);
            rec_at[i] = st.put(rec);
        }
        ia[i] = FxItemAgent{p.n, items ? sizeof(double) * (size_t)p.K * (size_t)(p.S - 1) : 0};
    }
    const long long forced = fx_predprob_scratch_forced.load(std::memory_order_relaxed);
    const std::vector<FxItemSegment> segs = fx_item_rounds(ia.data(), n_agents, forced > 0 ? (size_t)forced : FX_ITEM_SCRATCH_BYTES);
    const size_t R = segs.size();
    // the tiles x obstacles of all rows of a round choose the steps per chunk of each (fx_item_chunk_steps): as the candidates of
    // ONE obstacle, so that the rule sees the launch, not the agent
    std::vector<int64_t> tile_obst(R ? (size_t)segs.back().round + 1 : 0, 0), per_tile(R);
    std::vector<int32_t> cs(R), chunks(R);
    for (const FxItemSegment &g : segs)
        if (ia[g.agent].per_candidate_bytes) tile_obst[g.round] += (g.count + 63) / 64 * q[g.agent].K;
    for (size_t k = 0; k < R; k++) {
        const RiskPass &p = q[segs[k].agent];
        cs[k] = fx_predprob_chunk_steps(64 * tile_obst[segs[k].round], p.S, 1);
        chunks[k] = ia[segs[k].agent].per_candidate_bytes ? (std::max(p.S - 1, 1) + cs[k] - 1) / cs[k] : 0;
        per_tile[k] = (int64_t)chunks[k] * p.K;
    }
    FxItemTable tab;
    FX_TRY(fx_item_table(segs, ia.data(), n_agents, per_tile.data(), tab));
    const BatchTableAt t_at = batch_table_room<PredProbRow>(st, R, A);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(st.bytes.size()), o_step = lay.take(tab.scratch);
    const size_t o_prob = lay.take(sizeof(double) * rows_out), o_tot = lay.take(sizeof(double) * rows_out);
    const size_t o_best = lay.take(2 * sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    char *base;
    FX_TRY(risk_block(c, r, lay.size(), base));
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    std::vector<PredProbRow> rows(R, PredProbRow{});
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        PredProbRow &w = rows[k];
        predprob_args(q[g.agent], params + g.agent, n_pred[g.agent], w.a);
        w.a.ids = nullptr, w.a.rec = D(o_stage + rec_at[g.agent]);
        w.a.step = D(o_step + g.scratch_off), w.a.nb = tab.nb[k];
        w.a.prob = D(o_prob) + out_at[g.agent], w.a.prob_obs = nullptr, w.a.total = D(o_tot) + out_at[g.agent];
        w.first = g.first, w.count = g.count;
        w.cs = cs[k], w.chunks = chunks[k];
        w.item0 = tab.item0[k], w.fin0 = tab.fin0[k];
    }
    const PredProbBatchArgs t = batch_table_put(st, t_at, rows, tab, base + o_stage);
    HIP_TRY(hipMemcpyAsync(base + o_stage, st.bytes.data(), st.bytes.size(), hipMemcpyHostToDevice, c->stream));
    long long *d_best = reinterpret_cast<long long *>(base + o_best);
    HIP_TRY(fx_launch_predprob_batch(&t, tab.rounds.data(), (int)tab.rounds.size(), d_best, r->ev.e0, r->ev.e1, c->stream));
    if (out->prob && rows_out) HIP_TRY(hipMemcpyAsync(out->prob, base + o_prob, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    if (out->total && rows_out) HIP_TRY(hipMemcpyAsync(out->total, base + o_tot, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    std::vector<long long> best(2 * A);
    FX_TRY(risk_end(c, r, d_best, best.data(), 2 * A, &r->last_pp_ms));
    for (size_t i = 0; i < A; i++) {
        if (out->best_index) out->best_index[i] = risk_winner(q[i], best[2 * i]);
        if (out->best_cost) memcpy(out->best_cost + i, &best[2 * i + 1], sizeof(double));
    }
    return FX_OK;
}

// The responsibility pass over every candidate of several agents: the checks of
// fx_eval_responsibility_cost_agent (resp_check); every agent has the cost pass resp_check made of its parameters; beside the
// shared parts the stage holds the prediction entries and the per-agent argument blocks of the cost kernel and the re-sum.
// Runtime calls of a call with R rounds: 1 drain (a synchronisation), 1 ensure of the block, 1 copy up, 2 event records, 2 R + 3
// launches, 5 copies down (resp, total, ego_risk, obst_risk, best), 1 synchronisation.
extern "C" int32_t fx_eval_responsibility_cost_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params,
                                                     const FxRespCostParams *resp, const FxRespCostBatchOutputs *out) {
    std::vector<RiskPass> q;
    std::vector<FxRiskCostParams> cost;   // (sized in the check: the front has accepted n_agents by then)
    const bool have_out = out && out->resp && out->total && out->ego_risk && out->obst_risk && out->best_index && out->best_cost;
    const int rc = batch_front(c, (!params || !resp || !out) ? "params, resp or out is NULL" : nullptr, n_agents, agents, true, false, q,
                               [&](RiskPass &p, size_t i, int32_t agent) {
        cost.resize(q.size());
        return resp_check(p, c, agent, params + i, resp + i, 0, nullptr, have_out, cost[i]);   // (without ids it refuses a step that stored no bundle)
    });
    if (rc || n_agents == 0) return rc;
    const size_t A = (size_t)n_agents, none = ~(size_t)0;
    RiskStage st;
    std::vector<RiskBatchAgent> ag(A);
    std::vector<RespSumArgs> sums(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<int32_t> blk0(A);
    std::vector<size_t> pred_at(A, none);
    std::vector<double> rec;
    size_t rows_out = 0, col_doubles = 0;
    int64_t blocks = 0;
    for (size_t i = 0; i < A; i++) {
        RiskPass &p = q[i];
        RiskBatchAgent &b = ag[i];
        b.out_at = b.cout_at = rows_out, b.col_at = col_doubles, b.ci = (int)i;
        rows_out += (size_t)p.n;
        col_doubles += 4 * (size_t)p.K * (size_t)p.n;
        blk0[i] = (int32_t)blocks;
        blocks += (p.n + 255) / 256;
        b.at = risk_put_agent(st, p, rec);
        b.cost = risk_put_cost(st, p, &cost[i]);
        resp_sum_fill(p, resp + i, sums[i]);
        if (resp[i].prediction && sums[i].n_pred >= 0 && p.n > 0) pred_at[i] = st.put(resp[i].prediction, sizeof(double) * (size_t)p.n);
        ia[i] = risk_item_share(p, 7, b.sh);
    }
    if (blocks > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "%lld workgroups of candidates", (long long)blocks);
    std::vector<FxItemSegment> segs;
    FxItemTable tab;
    FX_TRY(risk_batch_table(ia, ag, segs, tab));
    const BatchTableAt t_at = batch_table_room<RiskBatchRow>(st, segs.size(), A);
    const size_t t_cost = st.room(sizeof(RiskCostArgs) * A), t_sum = st.room(sizeof(RespSumArgs) * A), t_blk0 = st.put(blk0);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(st.bytes.size()), o_part = lay.take(tab.scratch), o_col = lay.take(sizeof(double) * col_doubles);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out), o_occ = lay.take(sizeof(double) * rows_out);
    const size_t o_out = lay.take(sizeof(double) * 7 * rows_out), o_rresp = lay.take(sizeof(double) * rows_out);
    const size_t o_rtot = lay.take(sizeof(double) * rows_out), o_best = lay.take(2 * sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    char *base;
    FX_TRY(risk_block(c, r, lay.size(), base));
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    char *const d_stage = base + o_stage;
    std::vector<RiskCostArgs> cas(A, RiskCostArgs{});
    for (size_t i = 0; i < A; i++) {   // the per-agent argument blocks: the cost kernel's and the re-sum's
        const RiskPass &p = q[i];
        const RiskBatchAgent &b = ag[i];
        double *const po = D(o_out) + 7 * b.out_at;
        risk_cost_fill(p, &cost[i], risk_batch_cost_ptrs(d_stage, p, b, D(o_col) + b.col_at, po), cas[i]);
        RespSumArgs &rs = sums[i];
        rs.ids = nullptr;
        rs.resp = po + 4 * (size_t)p.n;
        rs.pred = pred_at[i] != none ? reinterpret_cast<const double *>(d_stage + pred_at[i]) : nullptr;
        rs.resp_out = D(o_rresp) + b.out_at, rs.total = D(o_rtot) + b.out_at;
    }
    memcpy(st.bytes.data() + t_cost, cas.data(), sizeof(RiskCostArgs) * A);
    memcpy(st.bytes.data() + t_sum, sums.data(), sizeof(RespSumArgs) * A);
    const std::vector<RiskBatchRow> rows = risk_fill_rows(segs, tab, q, ag, FX_FLAG_COSTED, d_stage, base + o_part, D(o_ego), D(o_obst),
                                                          D(o_occ), D(o_col));
    RiskBatchArgs t{};
    t.t = batch_table_put(st, t_at, rows, tab, d_stage);
    t.cost = reinterpret_cast<const RiskCostArgs *>(d_stage + t_cost);
    t.sum = reinterpret_cast<const RespSumArgs *>(d_stage + t_sum);
    t.blk0 = reinterpret_cast<const int32_t *>(d_stage + t_blk0);
    t.blocks = (int32_t)blocks;
    HIP_TRY(hipMemcpyAsync(d_stage, st.bytes.data(), st.bytes.size(), hipMemcpyHostToDevice, c->stream));
    long long *d_best = reinterpret_cast<long long *>(base + o_best);
    HIP_TRY(fx_launch_risk_batch(&t, tab.rounds.data(), (int)tab.rounds.size(), d_best, r->ev.e0, r->ev.e1, c->stream));
    if (rows_out) {
        const size_t bytes = sizeof(double) * rows_out;
        HIP_TRY(hipMemcpyAsync(out->resp, base + o_rresp, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->total, base + o_rtot, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->ego_risk, base + o_ego, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->obst_risk, base + o_obst, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<long long> best(2 * A);
    FX_TRY(risk_end(c, r, d_best, best.data(), 2 * A, &r->last_ms));
    for (size_t i = 0; i < A; i++) {
        out->best_index[i] = risk_winner(q[i], best[2 * i]);
        memcpy(out->best_cost + i, &best[2 * i + 1], sizeof(double));
    }
    return FX_OK;
}

// The id list of agent i of a call with lists, or none
static int64_t batch_n_ids(const int64_t *n_ids, size_t i) { return n_ids ? n_ids[i] : 0; }
static const int64_t *batch_ids(const int64_t *n_ids, const int64_t *const *ids, size_t i) { return (n_ids && ids) ? ids[i] : nullptr; }

// The plain risk pass of several agents, each with its own id list or none: the checks of
// fx_eval_risk_agent (risk_check: it resolves planes, ld, flags and the positions of listed candidates in a sparse set); nothing
// in the stage but the shared parts.  Runtime calls of a call with R rounds: 1 drain (a synchronisation), 1 ensure of the block, 1
// copy up, 2 event records, 2 R + 1 launches, 3 copies down (ego_risk, obst_risk, min_risk_index), 1 synchronisation.
extern "C" int32_t fx_eval_risk_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params, const int64_t *n_ids,
                                      const int64_t *const *ids, const FxRiskBatchOutputs *out) {
    std::vector<RiskPass> q;
    const char *const missing = (!params || !out) ? "params or out is NULL"
                                : (!out->ego_risk || !out->obst_risk || !out->min_risk_index) ? "an output pointer is NULL" : nullptr;
    const int rc = batch_front(c, missing, n_agents, agents, true, true, q, [&](RiskPass &p, size_t i, int32_t agent) {
        return risk_check(p, c, agent, params + i, batch_n_ids(n_ids, i), batch_ids(n_ids, ids, i), true, false);
    });
    if (rc || n_agents == 0) return rc;
    const size_t A = (size_t)n_agents;
    RiskStage st;
    std::vector<RiskBatchAgent> ag(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<double> rec;
    size_t rows_out = 0;
    for (size_t i = 0; i < A; i++) {
        RiskBatchAgent &b = ag[i];
        b.out_at = rows_out, b.col_at = b.cout_at = 0, b.ci = -1, b.cost = RiskCostAt{};
        rows_out += (size_t)q[i].n;
        b.at = risk_put_agent(st, q[i], rec);
        ia[i] = risk_item_share(q[i], 2, b.sh);
    }
    std::vector<FxItemSegment> segs;
    FxItemTable tab;
    FX_TRY(risk_batch_table(ia, ag, segs, tab));
    const BatchTableAt t_at = batch_table_room<RiskBatchRow>(st, segs.size(), A);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(st.bytes.size()), o_part = lay.take(tab.scratch);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out);
    const size_t o_idx = lay.take(sizeof(long long) * A);
    FxRiskState *r = q[0].r;
    char *base;
    FX_TRY(risk_block(c, r, lay.size(), base));
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    const std::vector<RiskBatchRow> rows = risk_fill_rows(segs, tab, q, ag, FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED, base + o_stage,
                                                          base + o_part, D(o_ego), D(o_obst), nullptr, nullptr);
    const RiskListBatchArgs t = batch_table_put(st, t_at, rows, tab, base + o_stage);
    HIP_TRY(hipMemcpyAsync(base + o_stage, st.bytes.data(), st.bytes.size(), hipMemcpyHostToDevice, c->stream));
    long long *d_idx = reinterpret_cast<long long *>(base + o_idx);
    HIP_TRY(fx_launch_risk_list_batch(&t, tab.rounds.data(), (int)tab.rounds.size(), d_idx, r->ev.e0, r->ev.e1, c->stream));
    if (rows_out) {
        HIP_TRY(hipMemcpyAsync(out->ego_risk, base + o_ego, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(out->obst_risk, base + o_obst, sizeof(double) * rows_out, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<long long> idx(A, -1);
    FX_TRY(risk_end(c, r, d_idx, idx.data(), A, &r->last_ms));
    for (size_t i = 0; i < A; i++) out->min_risk_index[i] = risk_winner(q[i], idx[i]);
    return FX_OK;
}

// The detail and cost passes of several agents, each with its own id list or none and its own cost parameters or none (DESIGN.md
// section 21): the checks of fx_eval_risk_costs_agent (risk_check with the detail flag, risk_cost_check); beside the shared parts
// the stage holds the cost kernel's argument blocks of the agents that have cost parameters and the column segments.  The columns
// and the principles lie per agent as the per-agent kernels' functions index them ([4][K][n] and [7][n]); the caller's are
// concatenated per column, so a last launch lays the column blocks out that way on the device, and the small principle block is
// laid out on the host.  Runtime calls of a call with R rounds: 1 drain (a synchronisation), 1 ensure of the block, 1 copy up, 2
// event records, 2 R + 4 launches (2 R + 1 where no agent has cost parameters and no column is asked for), at most 9 copies down
// (ego_risk, obst_risk, obst_harm_occ, the four columns, the principle block, the two arg-mins), 1 synchronisation.
extern "C" int32_t fx_eval_risk_costs_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const FxRiskParams *params,
                                            const FxRiskCostParams *const *cost, const int64_t *n_ids, const int64_t *const *ids,
                                            const FxRiskCostBatchOutputs *out) {
    std::vector<RiskPass> q;
    const int rc = batch_front(c, (!params || !out) ? "params or out is NULL" : nullptr, n_agents, agents, true, true, q,
                               [&](RiskPass &p, size_t i, int32_t agent) {
        const int rc_i = risk_check(p, c, agent, params + i, batch_n_ids(n_ids, i), batch_ids(n_ids, ids, i), true, true);
        return (!rc_i && cost && cost[i]) ? risk_cost_check(p, cost[i]) : rc_i;
    });
    if (rc || n_agents == 0) return rc;
    const size_t A = (size_t)n_agents;
    RiskStage st;
    std::vector<RiskBatchAgent> ag(A);
    std::vector<FxItemAgent> ia(A);
    std::vector<int32_t> blk0;
    std::vector<double> rec;
    size_t rows_out = 0, col_doubles = 0, rows_cost = 0;
    int64_t blocks = 0;
    for (size_t i = 0; i < A; i++) {
        RiskPass &p = q[i];
        RiskBatchAgent &b = ag[i];
        b.out_at = rows_out, b.col_at = col_doubles, b.cout_at = rows_cost, b.ci = -1, b.cost = RiskCostAt{};
        rows_out += (size_t)p.n;
        col_doubles += 4 * (size_t)p.K * (size_t)p.n;
        b.at = risk_put_agent(st, p, rec);
        if (cost && cost[i]) {
            b.ci = (int)blk0.size();
            blk0.push_back((int32_t)blocks);
            blocks += (p.n + 255) / 256;
            rows_cost += (size_t)p.n;
            b.cost = risk_put_cost(st, p, cost[i]);
        }
        ia[i] = risk_item_share(p, 7, b.sh);
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
    std::vector<FxItemSegment> segs;
    FxItemTable tab;
    FX_TRY(risk_batch_table(ia, ag, segs, tab));
    const BatchTableAt t_at = batch_table_room<RiskBatchRow>(st, segs.size(), A);
    const size_t t_cost = st.room(sizeof(RiskCostArgs) * NC), t_blk0 = st.put(blk0), t_seg = st.room(sizeof(RiskCopySeg) * NS),
                 t_sblk = st.put(seg_blk0);
    FxBlockLayout lay;
    const size_t o_stage = lay.take(st.bytes.size()), o_part = lay.take(tab.scratch), o_col = lay.take(sizeof(double) * col_doubles);
    const size_t o_cat = lay.take(any_col ? sizeof(double) * col_doubles : 0);
    const size_t o_ego = lay.take(sizeof(double) * rows_out), o_obst = lay.take(sizeof(double) * rows_out), o_occ = lay.take(sizeof(double) * rows_out);
    const size_t o_out = lay.take(sizeof(double) * 7 * rows_cost), o_idx = lay.take(sizeof(long long) * (A + NC));
    FxRiskState *r = q[0].r;
    char *base;
    FX_TRY(risk_block(c, r, lay.size(), base));
    auto D = [&](size_t o) { return reinterpret_cast<double *>(base + o); };
    char *const d_stage = base + o_stage;
    std::vector<RiskCostArgs> cas(NC, RiskCostArgs{});
    for (size_t i = 0; i < A; i++)   // the cost kernel's argument blocks of the agents that have cost parameters
        if (ag[i].ci >= 0)
            risk_cost_fill(q[i], cost[i], risk_batch_cost_ptrs(d_stage, q[i], ag[i], D(o_col) + ag[i].col_at, D(o_out) + 7 * ag[i].cout_at),
                           cas[(size_t)ag[i].ci]);
    if (NC) memcpy(st.bytes.data() + t_cost, cas.data(), sizeof(RiskCostArgs) * NC);
    const std::vector<RiskBatchRow> rows = risk_fill_rows(segs, tab, q, ag, FX_FLAG_VALID | FX_FLAG_FEASIBLE | FX_FLAG_RETURNED, d_stage,
                                                          base + o_part, D(o_ego), D(o_obst), D(o_occ), D(o_col));
    for (size_t k = 0; k < NS; k++) {   // plane k % 4 of agent k / 4: from its block to its place in that column of the call
        const size_t Kn = (size_t)q[k / 4].K * (size_t)q[k / 4].n, col_at = ag[k / 4].col_at;
        const RiskCopySeg g{D(o_col) + col_at + (k % 4) * Kn, D(o_cat) + (k % 4) * T + col_at / 4, (int64_t)Kn};
        memcpy(st.bytes.data() + t_seg + sizeof(RiskCopySeg) * k, &g, sizeof(g));
    }
    RiskCostBatchArgs t{};
    t.t = batch_table_put(st, t_at, rows, tab, d_stage);
    t.cost = reinterpret_cast<const RiskCostArgs *>(d_stage + t_cost);
    t.blk0 = reinterpret_cast<const int32_t *>(d_stage + t_blk0);
    t.n_cost = (int32_t)NC, t.blocks = (int32_t)blocks;
    t.seg = reinterpret_cast<const RiskCopySeg *>(d_stage + t_seg);
    t.seg_blk0 = reinterpret_cast<const int32_t *>(d_stage + t_sblk);
    t.n_seg = (int32_t)NS, t.seg_blocks = (int32_t)seg_blocks;
    HIP_TRY(hipMemcpyAsync(d_stage, st.bytes.data(), st.bytes.size(), hipMemcpyHostToDevice, c->stream));
    long long *d_idx = reinterpret_cast<long long *>(base + o_idx);
    HIP_TRY(fx_launch_risk_costs_batch(&t, tab.rounds.data(), (int)tab.rounds.size(), d_idx, d_idx + A, r->ev.e0, r->ev.e1, c->stream));
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
    FX_TRY(risk_end(c, r, d_idx, idx.data(), A + NC, &r->last_ms));
    r->last_rounds = (int32_t)tab.rounds.size();
    for (size_t i = 0; i < A; i++) {
        const RiskBatchAgent &b = ag[i];
        const size_t nn = (size_t)q[i].n;
        if (b.ci >= 0 && h_out)
            for (int k = 0; k < 7; k++)
                if (pr[k] && nn) memcpy(pr[k] + b.out_at, h_out.get() + 7 * b.cout_at + k * nn, sizeof(double) * nn);
        if (out->min_risk_index) out->min_risk_index[i] = risk_winner(q[i], idx[i]);
        if (out->min_cost_index) out->min_cost_index[i] = risk_winner(q[i], b.ci >= 0 ? idx[A + (size_t)b.ci] : -1);
    }
    return FX_OK;
}

// (hook of the tests, not part of fxplan.h: the rounds of scratch the last fx_eval_risk_costs_batch call took; -1 before the first)
extern "C" int32_t fx_last_risk_costs_batch_rounds(FxContext *c) { return (c && c->risk) ? c->risk->last_rounds : -1; }

extern "C" double fx_last_predprob_ms(FxContext *c) { return (c && c->risk) ? (double)c->risk->last_pp_ms : -1.0; }

extern "C" double fx_last_risk_ms(FxContext *c) { return (c && c->risk) ? (double)c->risk->last_ms : -1.0; }
