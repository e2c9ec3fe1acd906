// fx_api_risk.hip -- C-ABI of the trajectory risk (fx_risk_kernel.h): the obstacle tables of an agent and
// the risk pass with its arg-min over the materialised bundle of the last plan step; the reach sets of an agent and the detail /
// risk-cost pass.  Nothing of this runs in a plan step.
#include <cmath>
#include <vector>

#include "fx_context.h"
#include "fx_risk_args.h"

extern "C" hipError_t fx_launch_risk(const double *planes, int64_t ld, int S, int64_t n, const int64_t *ids, const uint32_t *flags,
                                     const double *rec, const double *obs, const double *pos, const double *yaw, const double *vo,
                                     int K, int P, const FxRiskParams *params, double *out_ego, double *out_obst, long long *out_idx,
                                     hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream);
// detail pass -> arg-min of ego + obst -> (cost != null) risk-cost kernel -> arg-min of the total into out_idx[1]
extern "C" hipError_t fx_launch_risk_costs(const double *planes, int64_t ld, int S, int64_t n, const int64_t *ids, const uint32_t *flags,
                                           const double *rec, const double *obs, const double *pos, const double *yaw, const double *vo,
                                           int K, int P, const FxRiskParams *params, double *out_ego, double *out_obst, double *col,
                                           double *out_occ, const RiskCostArgs *cost, long long *out_idx, hipEvent_t ev_start,
                                           hipEvent_t ev_stop, hipStream_t stream);

// the record layout of fx_risk_kernel.h (kept in step with it; the device header needs the HIP device compiler)
namespace {
constexpr int R_M0X = 0, R_SX = 6, R_SY = 7, R_RHO = 8, R_BRANCH = 9, R_NG = 10, R_VALID = 11, R_IV = 12, R_ASR = 16, R_A = 17,
              R_N1 = 18, R_N2 = 38, R_STRIDE = 58;
constexpr int O_LEN = 0, O_WID = 1, O_MASS = 2, O_CLS = 3, O_NPOS = 4, O_STRIDE = 8;
// Gauss-Legendre nodes on [-1, 1], positive half: 6, 12 and 20 points (Genz 2004)
const double kX6[3] = {0.9324695142031522, 0.6612093864662647, 0.2386191860831970};
const double kX12[6] = {0.9815606342467191, 0.9041172563704750, 0.7699026741943050,
                        0.5873179542866171, 0.3678314989981802, 0.1252334085114692};
const double kX20[10] = {0.9931285991850949, 0.9639719272779138, 0.9122344282513259, 0.8391169718222188, 0.7463319064601508,
                         0.6360536807265150, 0.5108670019508271, 0.3737060887154196, 0.2277858511416451, 0.07652652113349733};
}  // namespace

struct FxRiskAgent {
    int K = 0, P = 0;
    std::vector<double> pos, cov, cov_inv, yaw, v, obs;   // obs [K][O_STRIDE]
    std::vector<int32_t> n_pos, n_yaw, n_v;
    bool have_inv = false;
    // reach sets (fx_set_reach_sets_agent): entries index the K obstacles above, so new obstacles clear them
    std::vector<int32_t> rs_obs, rs_off, rs_step, rs_voff;
    std::vector<double> rs_verts;
};

struct FxRiskState {
    std::vector<FxRiskAgent> agents;
    double *d_buf = nullptr;
    size_t cap = 0;     // bytes
    char *d_cost = nullptr;   // fx_eval_risk_costs_agent's block, allocated on its first call
    size_t cap_cost = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float last_ms = 0.f;
};

void fx_risk_release(FxContext *c) {
    if (!c || !c->risk) return;
    FxRiskState *r = c->risk;
    if (r->d_buf) { (void)hipFree(r->d_buf); c->dev_bytes -= (int64_t)r->cap; }
    if (r->d_cost) { (void)hipFree(r->d_cost); c->dev_bytes -= (int64_t)r->cap_cost; }
    if (r->e0) (void)hipEventDestroy(r->e0);
    if (r->e1) (void)hipEventDestroy(r->e1);
    delete r;
    c->risk = nullptr;
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
    if (!c->risk) c->risk = new FxRiskState();
    FxRiskState *r = c->risk;
    if ((int)r->agents.size() < c->max_agents) r->agents.resize(c->max_agents);
    FxRiskAgent &a = r->agents[agent];
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
    a.obs.assign((size_t)K * O_STRIDE, 0.0);
    for (int k = 0; k < K; k++) {
        double *o = a.obs.data() + (size_t)k * O_STRIDE;
        o[O_LEN] = length[k];
        o[O_WID] = width[k];
        o[O_MASS] = mass[k];
        o[O_CLS] = (double)cls[k];
        o[O_NPOS] = (double)n_pos[k];
    }
    return FX_OK;
}

// the (obstacle, ego step) records: means, standardisation, |rho| branch and node terms -- once for all candidates
static void build_records(const FxRiskAgent &a, int S, bool mahalanobis, std::vector<double> &rec) {
    rec.assign((size_t)a.K * S * R_STRIDE, 0.0);
    for (int k = 0; k < a.K; k++) {
        const double len = a.obs[(size_t)k * O_STRIDE + O_LEN];
        for (int i = 1; i < S; i++) {
            double *q = rec.data() + ((size_t)k * S + i) * R_STRIDE;
            if (i >= a.n_pos[k]) continue;   // collision_probability.py:239: the prediction ends before ego point i
            q[R_VALID] = 1.0;
            const size_t p0 = (size_t)k * a.P + (i - 1);
            const double mx = a.pos[2 * p0], my = a.pos[2 * p0 + 1];
            const double yw = a.yaw[(size_t)k * a.P + i];   // yaw of prediction i, mean of prediction i - 1 (:182-185)
            const double dx = std::cos(yw) * len / 2.0, dy = std::sin(yw) * len / 2.0;
            const double m[6] = {mx, my, mx + dx, my + dy, mx - dx, my - dy};
            for (int u = 0; u < 6; u++) q[R_M0X + u] = m[u];
            if (mahalanobis) {
                for (int u = 0; u < 4; u++) q[R_IV + u] = a.cov_inv[4 * p0 + u];
                continue;
            }
            double cv[4] = {a.cov[4 * p0], a.cov[4 * p0 + 1], a.cov[4 * p0 + 2], a.cov[4 * p0 + 3]};
            if (cv[0] == 0.0 && cv[1] == 0.0 && cv[2] == 0.0 && cv[3] == 0.0) { cv[0] = 0.1; cv[1] = 0.0; cv[2] = 0.0; cv[3] = 0.1; }
            const double sx = std::sqrt(cv[0]), sy = std::sqrt(cv[3]);
            const double rho = cv[2] / sy / sx;   // mvnun: covar(2,1) / stdev(2) / stdev(1)
            q[R_SX] = sx;
            q[R_SY] = sy;
            q[R_RHO] = rho;
            const double ar = std::fabs(rho);
            const int ng = ar < 0.3 ? 3 : (ar < 0.75 ? 6 : 10);
            const double *x = ng == 3 ? kX6 : (ng == 6 ? kX12 : kX20);
            q[R_NG] = ng;
            if (rho == 0.0) {
                q[R_BRANCH] = 0;
            } else if (ar < 0.925) {
                q[R_BRANCH] = 1;
                const double asr = std::asin(rho) / 2.0;
                q[R_ASR] = asr;
                for (int j = 0; j < ng; j++) {
                    q[R_N1 + j] = std::sin(asr * (1.0 - x[j]));
                    q[R_N1 + ng + j] = std::sin(asr * (1.0 + x[j]));
                }
            } else if (ar < 1.0) {
                q[R_BRANCH] = 2;
                const double as = 1.0 - rho * rho, aa = std::sqrt(as), ah = aa / 2.0;
                q[R_ASR] = as;
                q[R_A] = aa;
                for (int j = 0; j < ng; j++) {
                    const double u0 = ah * (1.0 - x[j]), u1 = ah * (1.0 + x[j]);
                    q[R_N1 + j] = u0 * u0;
                    q[R_N1 + ng + j] = u1 * u1;
                    q[R_N2 + j] = std::sqrt(1.0 - q[R_N1 + j]);
                    q[R_N2 + ng + j] = std::sqrt(1.0 - q[R_N1 + ng + j]);
                }
            } else {
                q[R_BRANCH] = 3;
            }
        }
    }
}

extern "C" int32_t fx_eval_risk_agent(FxContext *c, int32_t agent, const FxRiskParams *params, int64_t n_ids, const int64_t *ids,
                                      double *ego_risk, double *obst_risk, int64_t *min_risk_index) {
    int rc = check_agent(c, agent);
    if (rc) return rc;
    const FxAgentSlot &s = c->slots[agent];
    if (!(s.mode & FX_MODE_WRITE_BUNDLE)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_BUNDLE");
    if (!params) return set_err(FX_ERR_INVALID_ARGUMENT, "params is NULL");
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
    if (n_ids < 0 || (n_ids > 0 && !ids)) return set_err(FX_ERR_INVALID_ARGUMENT, "ids inconsistent (n_ids=%lld)", (long long)n_ids);
    if (!ego_risk || !obst_risk || !min_risk_index) return set_err(FX_ERR_INVALID_ARGUMENT, "an output pointer is NULL");
    for (int64_t j = 0; ids && j < n_ids; j++)
        if (ids[j] < 0 || ids[j] >= s.C) return set_err(FX_ERR_INVALID_ARGUMENT, "candidate %lld out of range", (long long)ids[j]);
    if (!c->risk) c->risk = new FxRiskState();
    FxRiskState *r = c->risk;
    if ((int)r->agents.size() < c->max_agents) r->agents.resize(c->max_agents);
    const FxRiskAgent &a = r->agents[agent];
    const int S = s.S, K = a.K, P = a.P > 0 ? a.P : 1;
    const bool maha = p.prob_mode == FX_RISK_PROB_MAHALANOBIS;
    if (maha && K > 0 && !a.have_inv) return set_err(FX_ERR_INVALID_ARGUMENT, "Mahalanobis mode needs the inverse covariances");
    for (int k = 0; k < K; k++) {
        const int np = a.n_pos[k];
        if (a.n_yaw[k] < std::min(S, np) || a.n_v[k] < std::min(S - 1, np))
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: orientation_list (%d) / v_list (%d) shorter than calc_risk indexes "
                           "(%d / %d)", k, a.n_yaw[k], a.n_v[k], std::min(S, np), std::min(S - 1, np));
    }
    std::vector<double> rec;
    build_records(a, S, maha, rec);
    const int64_t n = ids ? n_ids : s.C;
    // one device block: rec | obs | pos | yaw | v | ids | ego | obst | index
    auto al = [](size_t b) { return align_up(b, 256); };
    const size_t b_rec = al(sizeof(double) * rec.size()), b_obs = al(sizeof(double) * std::max<size_t>(a.obs.size(), 1));
    const size_t b_pos = al(sizeof(double) * 2 * (size_t)K * P), b_kp = al(sizeof(double) * (size_t)K * P);
    const size_t b_ids = al(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1)), b_out = al(sizeof(double) * (size_t)std::max<int64_t>(n, 1));
    const size_t need = b_rec + b_obs + b_pos + 2 * b_kp + b_ids + 2 * b_out + 256;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tail_work = c->user_stream;
    if (need > r->cap) {
        if (r->d_buf) { HIP_TRY(hipFree(r->d_buf)); c->dev_bytes -= (int64_t)r->cap; r->d_buf = nullptr; r->cap = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r->d_buf), need));
        r->cap = need;
        c->dev_bytes += (int64_t)need;
    }
    if (!r->e0) { HIP_TRY(hipEventCreate(&r->e0)); HIP_TRY(hipEventCreate(&r->e1)); }
    char *base = reinterpret_cast<char *>(r->d_buf);
    double *d_rec = reinterpret_cast<double *>(base);
    double *d_obs = reinterpret_cast<double *>(base + b_rec);
    double *d_pos = reinterpret_cast<double *>(base + b_rec + b_obs);
    double *d_yaw = reinterpret_cast<double *>(base + b_rec + b_obs + b_pos);
    double *d_v = reinterpret_cast<double *>(base + b_rec + b_obs + b_pos + b_kp);
    int64_t *d_ids = reinterpret_cast<int64_t *>(base + b_rec + b_obs + b_pos + 2 * b_kp);
    double *d_ego = reinterpret_cast<double *>(base + b_rec + b_obs + b_pos + 2 * b_kp + b_ids);
    double *d_obst = reinterpret_cast<double *>(base + b_rec + b_obs + b_pos + 2 * b_kp + b_ids + b_out);
    long long *d_idx = reinterpret_cast<long long *>(base + b_rec + b_obs + b_pos + 2 * b_kp + b_ids + 2 * b_out);
    if (K > 0) {
        HIP_TRY(hipMemcpyAsync(d_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_obs, a.obs.data(), sizeof(double) * a.obs.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_pos, a.pos.data(), sizeof(double) * a.pos.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_yaw, a.yaw.data(), sizeof(double) * a.yaw.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_v, a.v.data(), sizeof(double) * a.v.size(), hipMemcpyHostToDevice, c->stream));
    }
    if (ids && n > 0) HIP_TRY(hipMemcpyAsync(d_ids, ids, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(fx_launch_risk(c->h_probs[agent].planes, s.ld, S, n, ids ? d_ids : nullptr, c->d_flags + s.cand_off, d_rec, d_obs, d_pos,
                           d_yaw, d_v, K, P, &p, d_ego, d_obst, d_idx, r->e0, r->e1, c->stream));
    long long idx = -1;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(ego_risk, d_ego, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(obst_risk, d_obst, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(&idx, d_idx, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->e0, r->e1));
    *min_risk_index = (int64_t)idx;
    return FX_OK;
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
    if (!c->risk) c->risk = new FxRiskState();
    FxRiskState *r = c->risk;
    if ((int)r->agents.size() < c->max_agents) r->agents.resize(c->max_agents);
    FxRiskAgent &a = r->agents[agent];
    a.rs_obs.assign(entry_obs, entry_obs + n_entries);
    a.rs_off.clear();
    if (n_entries > 0) a.rs_off.assign(entry_part_off, entry_part_off + n_entries + 1);
    a.rs_step.assign(part_step, part_step + n_parts);
    a.rs_voff.clear();
    if (n_parts > 0) a.rs_voff.assign(part_vert_off, part_vert_off + n_parts + 1);
    a.rs_verts.assign(verts, verts + 2 * (size_t)n_verts);
    return FX_OK;
}

extern "C" int32_t fx_eval_risk_costs_agent(FxContext *c, int32_t agent, const FxRiskParams *params, const FxRiskCostParams *cost,
                                            int64_t n_ids, const int64_t *ids, const FxRiskOutputs *out) {
    int rc = check_agent(c, agent);
    if (rc) return rc;
    const FxAgentSlot &s = c->slots[agent];
    if (!(s.mode & FX_MODE_WRITE_BUNDLE)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_BUNDLE");
    if (!params || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "params or out is NULL");
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
    if (n_ids < 0 || (n_ids > 0 && !ids)) return set_err(FX_ERR_INVALID_ARGUMENT, "ids inconsistent (n_ids=%lld)", (long long)n_ids);
    for (int64_t j = 0; ids && j < n_ids; j++)
        if (ids[j] < 0 || ids[j] >= s.C) return set_err(FX_ERR_INVALID_ARGUMENT, "candidate %lld out of range", (long long)ids[j]);
    if (!c->risk) c->risk = new FxRiskState();
    FxRiskState *r = c->risk;
    if ((int)r->agents.size() < c->max_agents) r->agents.resize(c->max_agents);
    const FxRiskAgent &a = r->agents[agent];
    const int S = s.S, K = a.K, P = a.P > 0 ? a.P : 1;
    const bool maha = p.prob_mode == FX_RISK_PROB_MAHALANOBIS;
    if (maha && K > 0 && !a.have_inv) return set_err(FX_ERR_INVALID_ARGUMENT, "Mahalanobis mode needs the inverse covariances");
    for (int k = 0; k < K; k++) {
        const int np = a.n_pos[k];
        if (std::min(S - 1, np) <= 0)
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: min(S - 1, len(pos_list)) == 0 (calc_risk takes the maximum of an empty "
                           "list upstream)", k);
        if (a.n_yaw[k] < std::min(S, np) || a.n_v[k] < std::min(S - 1, np))
            return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle %d: orientation_list (%d) / v_list (%d) shorter than calc_risk indexes "
                           "(%d / %d)", k, a.n_yaw[k], a.n_v[k], std::min(S, np), std::min(S - 1, np));
    }
    const bool reach = cost && cost->responsibility_mode == FX_RISK_RESP_REACH_SET;
    if (cost) {
        if (cost->boundary_mode < FX_RISK_BOUNDARY_ZERO || cost->boundary_mode > FX_RISK_BOUNDARY_STEP ||
            (cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY && !cost->boundary_harm))
            return set_err(FX_ERR_INVALID_ARGUMENT, "boundary_mode %d", cost->boundary_mode);
        if (cost->responsibility_mode < FX_RISK_RESP_NONE || cost->responsibility_mode > FX_RISK_RESP_REACH_SET ||
            (cost->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && K > 0 && !cost->responsibility))
            return set_err(FX_ERR_INVALID_ARGUMENT, "responsibility_mode %d", cost->responsibility_mode);
        if (reach) {
            for (size_t e = 0; e < a.rs_obs.size(); e++)
                if (a.rs_obs[e] >= K)
                    return set_err(FX_ERR_INVALID_ARGUMENT, "reach-set entry %d: obstacle index %d is not among the %d predictions", (int)e,
                                   a.rs_obs[e], K);
            for (size_t q = 0; q < a.rs_step.size(); q++)
                if (a.rs_step[q] >= S)
                    return set_err(FX_ERR_INVALID_ARGUMENT, "reach-set part %d: step index %d outside the horizon (S=%d)", (int)q, a.rs_step[q], S);
        }
    }
    std::vector<double> rec;
    build_records(a, S, maha, rec);
    const int64_t n = ids ? n_ids : s.C;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), KP = (size_t)K * P;
    const size_t nE = reach ? a.rs_obs.size() : 0, nP = reach ? a.rs_step.size() : 0, nV = reach ? a.rs_verts.size() / 2 : 0;
    // one device block; every part 256-byte aligned
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += align_up(std::max<size_t>(bytes, 8), 256); return o; };
    const size_t o_rec = take(sizeof(double) * rec.size()), o_obs = take(sizeof(double) * a.obs.size());
    const size_t o_pos = take(sizeof(double) * 2 * KP), o_yaw = take(sizeof(double) * KP), o_v = take(sizeof(double) * KP);
    const size_t o_ids = take(sizeof(int64_t) * n1), o_ego = take(sizeof(double) * n1), o_obst = take(sizeof(double) * n1);
    const size_t o_occ = take(sizeof(double) * n1), o_col = take(sizeof(double) * 4 * (size_t)K * n1);
    const size_t o_out = take(sizeof(double) * 7 * n1), o_bh = take(sizeof(double) * n1), o_resp = take(sizeof(double) * (size_t)K);
    const size_t o_eobs = take(sizeof(int32_t) * nE), o_eoff = take(sizeof(int32_t) * (nE + 1));
    const size_t o_pst = take(sizeof(int32_t) * nP), o_voff = take(sizeof(int32_t) * (nP + 1)), o_vert = take(sizeof(double) * 2 * nV);
    const size_t o_idx = take(2 * sizeof(long long));
    const size_t need = off;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tail_work = c->user_stream;
    if (need > r->cap_cost) {
        if (r->d_cost) { HIP_TRY(hipFree(r->d_cost)); c->dev_bytes -= (int64_t)r->cap_cost; r->d_cost = nullptr; r->cap_cost = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r->d_cost), need));
        r->cap_cost = need;
        c->dev_bytes += (int64_t)need;
    }
    if (!r->e0) { HIP_TRY(hipEventCreate(&r->e0)); HIP_TRY(hipEventCreate(&r->e1)); }
    char *base = r->d_cost;
    auto D = [base](size_t o) { return reinterpret_cast<double *>(base + o); };
    auto I = [base](size_t o) { return reinterpret_cast<int32_t *>(base + o); };
    auto up = [&](size_t o, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    if (K > 0) {
        HIP_TRY(up(o_rec, rec.data(), sizeof(double) * rec.size()));
        HIP_TRY(up(o_obs, a.obs.data(), sizeof(double) * a.obs.size()));
        HIP_TRY(up(o_pos, a.pos.data(), sizeof(double) * a.pos.size()));
        HIP_TRY(up(o_yaw, a.yaw.data(), sizeof(double) * a.yaw.size()));
        HIP_TRY(up(o_v, a.v.data(), sizeof(double) * a.v.size()));
    }
    if (ids && n > 0) HIP_TRY(up(o_ids, ids, sizeof(int64_t) * n));
    int64_t *d_ids = ids ? reinterpret_cast<int64_t *>(base + o_ids) : nullptr;
    RiskCostArgs ca{};
    if (cost) {
        if (cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY && n > 0) HIP_TRY(up(o_bh, cost->boundary_harm, sizeof(double) * n));
        if (cost->responsibility_mode == FX_RISK_RESP_ACTION_SPACE && K > 0) HIP_TRY(up(o_resp, cost->responsibility, sizeof(double) * K));
        if (reach && nE > 0) {
            HIP_TRY(up(o_eobs, a.rs_obs.data(), sizeof(int32_t) * nE));
            HIP_TRY(up(o_eoff, a.rs_off.data(), sizeof(int32_t) * (nE + 1)));
            if (nP > 0) {
                HIP_TRY(up(o_pst, a.rs_step.data(), sizeof(int32_t) * nP));
                HIP_TRY(up(o_voff, a.rs_voff.data(), sizeof(int32_t) * (nP + 1)));
                HIP_TRY(up(o_vert, a.rs_verts.data(), sizeof(double) * 2 * nV));
            }
        }
        ca.col = D(o_col);
        ca.n = n;
        ca.ids = d_ids;
        ca.flags = c->d_flags + s.cand_off;
        ca.planes = c->h_probs[agent].planes;
        ca.ld = s.ld;
        ca.S = S;
        ca.K = K;
        ca.bh_in = cost->boundary_mode == FX_RISK_BOUNDARY_ARRAY ? D(o_bh) : nullptr;
        ca.bstep = (cost->boundary_mode == FX_RISK_BOUNDARY_STEP && (s.mode & FX_MODE_ROAD_BOUNDARY)) ? c->d_bstep + s.cand_off : nullptr;
        ca.bh_c = cost->boundary_c;
        ca.bh_s = cost->boundary_s;
        ca.resp_mode = cost->responsibility_mode;
        ca.n_entries = (int32_t)nE;
        ca.resp = D(o_resp);
        ca.entry_obs = I(o_eobs);
        ca.entry_off = I(o_eoff);
        ca.part_step = I(o_pst);
        ca.vert_off = I(o_voff);
        ca.verts = D(o_vert);
        for (int q = 0; q < 5; q++) ca.w[q] = cost->weights[q];
        ca.eps = cost->maximin_eps;
        ca.scale = cost->maximin_scale;
        ca.out = D(o_out);
    }
    long long *d_idx = reinterpret_cast<long long *>(base + o_idx);
    HIP_TRY(fx_launch_risk_costs(c->h_probs[agent].planes, s.ld, S, n, d_ids, c->d_flags + s.cand_off, D(o_rec), D(o_obs), D(o_pos),
                                 D(o_yaw), D(o_v), K, P, &p, D(o_ego), D(o_obst), D(o_col), D(o_occ), cost ? &ca : nullptr, d_idx,
                                 r->e0, r->e1, c->stream));
    auto down = [&](double *dst, size_t o, size_t count) {
        return (dst && count) ? hipMemcpyAsync(dst, base + o, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    const size_t nn = (size_t)n, Kn = (size_t)K * nn;
    HIP_TRY(down(out->ego_risk, o_ego, nn));
    HIP_TRY(down(out->obst_risk, o_obst, nn));
    HIP_TRY(down(out->obst_harm_occ, o_occ, nn));
    double *const cols[4] = {out->ego_risk_max, out->obst_risk_max, out->ego_harm_max, out->obst_harm_max};
    for (int q = 0; q < 4; q++) HIP_TRY(down(cols[q], o_col + sizeof(double) * q * Kn, Kn));
    if (cost) {
        double *const pr[7] = {out->bayes, out->equality, out->maximin, out->ego, out->responsibility, out->total, out->boundary_harm};
        for (int q = 0; q < 7; q++) HIP_TRY(down(pr[q], o_out + sizeof(double) * q * nn, nn));
    }
    long long idx[2] = {-1, -1};
    HIP_TRY(hipMemcpyAsync(idx, d_idx, sizeof(idx), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&r->last_ms, r->e0, r->e1));
    if (out->min_risk_index) *out->min_risk_index = (int64_t)idx[0];
    if (out->min_cost_index) *out->min_cost_index = cost ? (int64_t)idx[1] : -1;
    return FX_OK;
}

extern "C" double fx_last_risk_ms(FxContext *c) { return (c && c->risk) ? (double)c->risk->last_ms : -1.0; }
