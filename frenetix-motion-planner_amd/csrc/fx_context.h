// fx_context.h -- what the translation units of the C-ABI share: the context and its helpers (the launchers: fx_launch.h).
//   fx_api.hip           context life cycle, settings, measurement hooks
//   fx_api_step.hip      upload, evaluation (launch policy: fx_policy.h), results, state updates, winner package, batched plan calls
//   fx_api_exchange.hip  survivor exchange inside the library (RCCL)
//   fx_api_host.hip      host geometry of the callers either side of the path, read-back
//   fx_api_risk.hip      trajectory risk and risk costs beside the plan step
//   fx_api_materialise.hip  listed candidates of a step re-walked into a sparse set, its read-back and package
//   fx_api_sort.hip      stable cost order of all candidates beside the step, read back by rank
//   fx_api_rescore.hip   the step re-scored under other cost weights, one agent or a batch; the device view of the raw cost rows
//   fx_api_hypotheses.hip  the step's obstacle stage re-evaluated under other prediction sets
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <atomic>

#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <tuple>
#include <vector>
#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>

#include "fx_launch.h"
#include "fx_owner.h"

// state updates up to this many bytes are staged by a copy kernel reading the mapped pinned block, larger ones by the DMA engine
#define FX_STAGE_KERNEL_MAX ((size_t)1 << 20)
#define FX_STAGE_HOST_MAX ((size_t)4 << 20)     // host writes into the device arena (large BAR): ~50 GB/s of posted writes
#define FX_PUB_MAX 16384  // doubles: 8 ranks x 64 survivors x 2 x 16 agents

struct FxAgentSlot {
    int64_t C = 0, ld = 0, cand_off = 0;  // cand_off: offset of this agent in the per-candidate arrays
    int32_t S = 0, n_cost = 0, n_blocks = 0;
    uint32_t mode = 0;
    // where the step-dependent inputs of this agent sit in the pinned staging block (fx_update_state rewrites them in
    // place); (size_t)-1 = not present
    size_t off_t = (size_t)-1, off_v = (size_t)-1, off_d = (size_t)-1, off_ref = (size_t)-1;
    size_t off_pos = (size_t)-1, off_cov = (size_t)-1, off_npred = (size_t)-1, off_hull = (size_t)-1, off_nhull = (size_t)-1;
    size_t off_rec = (size_t)-1, off_pm = (size_t)-1, off_hm = (size_t)-1, off_hot = (size_t)-1;
    size_t dyn_end = 0;   // end of this agent's step-dependent inputs that the walk reads every step
    size_t raw_end = 0;   // end of the raw predictions behind them
    int32_t nT = 0, nV = 0, nD = 0, K = 0, P = 0, M = 0;
    bool have_hull = false, want_collision = false;
};

void fx_risk_release(struct FxRiskState *r);       // (fx_api_risk.hip)
void fx_sparse_release(struct FxSparseState *s);   // (fx_api_materialise.hip)
void fx_sort_release(struct FxSortState *s);       // (fx_api_sort.hip)
void fx_rescore_release(struct FxRescoreState *s);   // (fx_api_rescore.hip)
void fx_hyp_release(struct FxHypState *s);           // (fx_api_hypotheses.hip)

struct FxContext {
    int device = 0;
    FxStream stream;             // the first owner: everything below is given back before the stream is destroyed
    int64_t dev_bytes = 0;       // device memory held (fx_device_bytes): kept by the device arrays below and by the passes' blocks
    // timing ring: per timed step (start, evaluation end, step end) events; elapsed times are read lazily, so a
    // timed step never waits for its own events
    struct TimeSlot {
        FxEvent e0, e_eval, e_end, e_obs0, e_obs1;
        bool eval_launched = false, fused = false, fetched = false, obst_timed = false;
        float step_ms = 0.f, eval_ms = 0.f, obst_ms = 0.f;
    };
    static constexpr int kTimeRing = 256;
    TimeSlot ring[kTimeRing];
    long long n_timed = 0;       // timed steps so far (slot = (n_timed - 1) % kTimeRing is the latest)
    long long n_steps = 0;       // evaluations so far
    int timing_every = 1;        // time every n-th step
    // capacities
    int32_t max_agents = 1;                // (the others: caps)
    // input arena
    size_t in_bytes = 0;
    FxPinned<char> h_in;       // pinned + mapped (the staging kernel reads it through h_in.dev)
    int stage_mode = 0;        // 0 auto: kernel copy up to FX_STAGE_KERNEL_MAX bytes, DMA above; 1 DMA; 2 kernel; 3 host writes into
                               // device memory -- OPT-IN, or fail (FX_STAGE=dma|kernel|bar)
    bool user_stream = false;  // fx_set_stream handed in a caller's stream: what else is queued on it is unknown
    bool bar_ok = false;       // FX_STAGE=bar and the input arena d_in is mapped into this process (large BAR), host stores reach it
                               // and a kernel that had the lines cached sees a second write (probed at fx_create)
    volatile uint32_t *hdp_flush = nullptr;   // the device's HDP flush register (hipDeviceAttributeHdpMemFlushCntl), written behind host stores
    int stage_path = 0;        // how the latest inputs reached the device: 1 DMA copy, 2 staging kernel, 3 host writes
    FxDeviceArray<char> d_in{&dev_bytes};
    // problems
    DevProblem *h_probs = nullptr;  // [max_agents], the front of the pinned staging block h_in ...
    DevProblem *d_probs = nullptr;  // ... and of its device twin d_in: problems and inputs travel in ONE copy
    size_t probs_bytes = 0;
    // outputs
    FxDeviceArray<double> d_cost{&dev_bytes};
    FxDeviceArray<double> d_cost_tail{&dev_bytes};     // [total_ld] cost terms behind the prediction term (obstacle stage as its own kernel)
    // obstacle kernel scratch (allocated on first use): partial sums [chunks][ld], collision ballots [chunks][tiles], tile tickets
    FxDeviceArray<double> d_obs_part{&dev_bytes};
    FxDeviceArray<unsigned long long> d_obs_colm{&dev_bytes};
    FxDeviceArray<unsigned int> d_obs_ticket{&dev_bytes};
    FxDeviceArray<int32_t> d_obs_list{&dev_bytes};     // [total_ld] the walk's list of costed candidates per agent (obstacle stage as its own kernel)
    FxDeviceArray<uint32_t> d_flags{&dev_bytes};
    FxDeviceArray<double> d_costmap{&dev_bytes};
    FxDeviceArray<double> d_coeffs{&dev_bytes};
    FxDeviceArray<int32_t> d_trajlen{&dev_bytes};
    FxDeviceArray<int32_t> d_bstep{&dev_bytes};       // [total_ld] first road-boundary step per candidate
    FxPinned<char> h_bound;                // road-boundary pieces / bins / items (grown on demand) ...
    FxDeviceArray<char> d_bound{&dev_bytes};   // ... and their device twin, of the same size
    FxDeviceArray<double> d_planes{&dev_bytes};   // the bundle (grown on demand)
    FxDeviceArray<double> d_part_cost{&dev_bytes};
    FxDeviceArray<int64_t> d_part_idx{&dev_bytes};
    FxDeviceArray<unsigned long long> d_counters{&dev_bytes};  // [max_agents][FX_CNT_COUNT]
    FxPinned<unsigned long long> h_counters;   // pinned + mapped: [max_agents][FX_CNT_COUNT + 1], last word = sequence
    unsigned long long seq = 0;
    // survivor exchange inside the library (fx_comm_init): an RCCL communicator of this context's own, the gathered winners
    void *comm = nullptr;                  // ncclComm_t
    int comm_rank = 0, comm_world = 0;
    int comm_agents = 0;                   // agent rows EVERY rank contributes to an exchange (fx_comm_set_agents; default max_agents)
    int comm_rows_clean = 0;               // send-buffer rows [comm_rows_clean, comm_agents) hold "no survivor"
    int comm_k_clean = 0;                  // ... for this k (0: the winner buffer)
    bool comm_init_failed = false;         // an fx_comm_init on this context timed out: never retried
    int exchange_mode = 0;                 // fx_set_exchange_mode: 0 receive in device memory + publication kernel, 1 receive straight in the pinned block
    FxDeviceArray<double> d_gather{&dev_bytes};   // [world][max_agents][2] (grown to [world][max_agents][2 k] by the top-k exchange)
    FxDeviceArray<double> d_xsend{&dev_bytes};    // [max_agents][2][64]: a rank's survivors, [cost n k | index n k], the all-gather's send buffer
    int timeout_ms = 20000;                // bound of every host wait on device work (fx_set_timeout_ms)
    bool timed_out = false;                // a wait ran out: the stream may never drain, the context refuses further steps
    FxPinned<double> h_pub;                // pinned + mapped [FX_PUB_MAX + 1]: published buffer, last word = sequence
    unsigned long long pub_seq = 0;
    int pub_n = 0;
    double *dev_winner = nullptr;          // caller-owned device buffer [n_agents][2] the selection kernel also fills
    bool in_flight = false;                // work enqueued whose completion the host has not observed yet
    bool tail_work = false;                // work queued behind the evaluation whose completion NO sequence word reports (top-k, publication,
                                           // exchange) or a caller's own stream (fx_set_stream): cleared only by a stream synchronise --
                                           // fx_finish_batch clears in_flight when the evaluation's words arrive, which says nothing about these
    FxDeviceArray<double> d_topk_cost{&dev_bytes};
    FxDeviceArray<long long> d_topk_idx{&dev_bytes};
    FxDeviceArray<double> d_topk_scr_cost{&dev_bytes};     // [max_agents][64 slices][64]
    FxDeviceArray<long long> d_topk_scr_idx{&dev_bytes};
    FxPinned<double> h_topk_cost;
    // winner package (fx_set_package): pinned + mapped [max_agents][pkg_stride] doubles the package kernel fills behind the selection
    FxPinned<double> h_pkg;
    int pkg_stride = 0, pkg_plane_rows = 0;
    FxDeviceArray<double> d_winner_own{&dev_bytes};   // [max_agents][2]: the winner stays device-resident for the package kernel
    bool package_enabled = false;
    FxPinned<double> h_cand;   // pinned staging of fx_read_candidate_agent: planes | coeffs | raw costs | cost | traj_len | flags
    // chunk of fx_read_candidates_agent (FX_READ_CHUNK_BYTES each, allocated on its first call): ids | packed records, on the device
    // and pinned
    FxDeviceArray<char> d_cands{&dev_bytes};
    FxPinned<char> h_cands;
    FxPinned<long long> h_topk_idx;
    // current step
    int n_agents = 0;
    std::vector<FxAgentSlot> slots;
    bool uploaded = false, evaluated = false;
    size_t in_used = 0;                    // bytes of the staging block the last upload filled
    size_t dirty_lo = (size_t)-1, dirty_hi = 0;  // staging range rewritten by fx_update_state, copied by the next evaluation
    bool probs_dirty = false;
    // launch policy (fx_policy.h): what callers and experiments force, what the last upload decided, what the last evaluation launched
    FxForce force;
    FxCaps caps;
    FxStepPlan plan;
    std::vector<FxAgentPlan> plan_rows;    // [max_agents], plan.agents
    FxLaunchPlan launch;
    int64_t last_live = -1;                // costed candidates of the previous step's agents (max): sizes the one-launch step's obstacle items
    FxDeviceArray<unsigned long long> d_bar{&dev_bytes};   // the one-launch step's two grid barriers' counter + release-flag blocks, monotonic
    unsigned long long bar_base = 0;       // their value before the next launch
    int timing = FX_TIMING_OFF;
    bool timed_step = false;
    // the states of the passes beside the step, created on first use; each is deleted where its type is complete
    std::unique_ptr<FxRiskState, void (*)(FxRiskState *)> risk{nullptr, fx_risk_release};         // trajectory risk: obstacle tables and buffers
    std::unique_ptr<FxSparseState, void (*)(FxSparseState *)> sparse{nullptr, fx_sparse_release};   // sparse sets of listed candidates
    std::unique_ptr<FxSortState, void (*)(FxSortState *)> sort{nullptr, fx_sort_release};           // cost order of all candidates
    std::unique_ptr<FxRescoreState, void (*)(FxRescoreState *)> rescore{nullptr, fx_rescore_release};   // re-score under other weights
    std::unique_ptr<FxHypState, void (*)(FxHypState *)> hyp{nullptr, fx_hyp_release};                   // the obstacle stage under other predictions
};

// An agent's sparse set as its consumers see it (fx_api_materialise.hip): the structure-of-arrays rows of
// the n listed candidates, column = position in the ascending, de-duplicated list `ids`
struct FxSparseView {
    const int64_t *ids;   // [n] host, ascending
    int64_t n, ld;
    const double *planes, *coeffs, *costmap, *cost;   // device
    const uint32_t *flags;
    const int32_t *traj_len, *bound_step;
};
// the valid set of `agent`, or false: none materialised since the last evaluation, upload or state update
bool fx_sparse_view(FxContext *c, int32_t agent, FxSparseView *v);
// positions of the listed candidates in the set; false when one of them is not in it
bool fx_sparse_positions(const FxSparseView &v, int64_t n, const int64_t *ids, std::vector<int64_t> &pos);

int fx_gather_rows(FxContext *c, const GatherArgs &ga, int64_t n, const int64_t *ids, double *planes, double *coeffs13, int32_t *traj_len,
                   double *raw_costs, double *cost, uint32_t *flags, int32_t *boundary_step);   // (fx_api_host.hip)
void fx_package_derive(const DevProblem &d, int S, double yaw_rate0, double *block);             // (fx_api_step.hip)

extern "C" int32_t fx_wait_word(const volatile unsigned long long *word, unsigned long long expected, int32_t timeout_ms);   // (fx_api.hip)



// wait for a word of this context's pinned blocks; a timeout poisons the context (its stream may never drain)
inline int wait_seq(FxContext *c, const volatile unsigned long long *word, unsigned long long expected) {
    const int rc = fx_wait_word(word, expected, c->timeout_ms);
    if (rc == FX_ERR_TIMEOUT) c->timed_out = true;
    return rc;
}

// per-step obstacle masks: one 64-bit word per 64 obstacles, word-major ([word][step]) so that the first word is the whole
// table for K <= 64 (the only case the grid kernel's staged obstacle path handles)
inline int mask_words(int K) { return K > 0 ? (K + 63) / 64 : 1; }

inline size_t input_bytes_for(int64_t cand, int S, int M, int K, int Pn, bool matrix) {
    size_t b = 0;
    b += align_up(sizeof(double) * 5 * S, 256);
    b += align_up(sizeof(double) * 3 * 4096, 256);              // t/v/d ranges
    if (matrix) b += align_up(sizeof(double) * 13 * (size_t)cand, 256);
    b += align_up(sizeof(double) * FX_REF_FIELDS * (size_t)M, 256);
    b += align_up(sizeof(double) * 2 * (size_t)K * Pn, 256);
    b += align_up(sizeof(double) * 4 * (size_t)K * Pn, 256);
    b += align_up(sizeof(double) * 6 * (size_t)K * (Pn > 0 ? Pn : 1), 256);
    b += align_up(sizeof(double) * 12 * (size_t)K * S, 256) + 2 * align_up(sizeof(unsigned long long) * S * (size_t)mask_words(K), 256);
    b += align_up(sizeof(double) * FX_HOT_STRIDE * (size_t)K * S, 256);  // hot obstacle table
    b += 2 * align_up(sizeof(int32_t) * (size_t)K, 256);
    b += align_up(sizeof(double) * 2 * (size_t)K, 256);           // dto positions (<= K)
    return b + 4096;
}

struct Arena {
    char *h, *d;
    size_t off, cap;
    template <typename T>
    const T *put(const T *src, size_t n, bool *ok) {
        size_t bytes = align_up(n * sizeof(T), 256);
        if (off + bytes > cap) { *ok = false; return nullptr; }
        if (n && src) memcpy(h + off, src, n * sizeof(T));
        const T *dp = reinterpret_cast<const T *>(d + off);
        off += bytes;
        return dp;
    }
    template <typename T>
    T *host_slot(size_t n, const T **dev, bool *ok) {
        size_t bytes = align_up(n * sizeof(T), 256);
        if (off + bytes > cap) { *ok = false; return nullptr; }
        T *hp = reinterpret_cast<T *>(h + off);
        *dev = reinterpret_cast<const T *>(d + off);
        off += bytes;
        return hp;
    }
};

// elapsed times of one ring slot (waits for the slot's last event if it is still pending)
inline int fetch_slot(FxContext *c, FxContext::TimeSlot &t) {
    if (t.fetched) return FX_OK;
    hipEvent_t end = t.fused ? t.e_eval : t.e_end;
    HIP_TRY(hipEventSynchronize(end));
    HIP_TRY(hipEventElapsedTime(&t.step_ms, t.e0, end));
    if (t.eval_launched) HIP_TRY(hipEventElapsedTime(&t.eval_ms, t.e0, t.e_eval));
    else t.eval_ms = 0.f;
    t.obst_ms = 0.f;
    if (t.obst_timed) HIP_TRY(hipEventElapsedTime(&t.obst_ms, t.e_obs0, t.e_obs1));
    t.fetched = true;
    return FX_OK;
}

inline int validate(const FxProblem *p) {
    if (!p) return set_err(FX_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (p->N < 1 || p->N + 1 > FX_MAX_SAMPLES) return set_err(FX_ERR_INVALID_ARGUMENT, "N=%d outside [1,%d]", p->N, FX_MAX_SAMPLES - 1);
    if (!(p->dt > 0)) return set_err(FX_ERR_INVALID_ARGUMENT, "dt must be > 0");
    if (p->M < 2 || !p->ref_pos || !p->ref_x || !p->ref_y || !p->ref_nx || !p->ref_ny || !p->ref_theta || !p->ref_curv ||
        !p->ref_curv_d)
        return set_err(FX_ERR_NOT_READY, "reference path not set (M=%d)", p->M);
    if (!p->tpow) return set_err(FX_ERR_INVALID_ARGUMENT, "tpow table missing");
    if (p->sampling_matrix) {
        if (p->n_rows < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_rows < 0");
    } else {
        if (p->nT < 0 || p->nV < 0 || p->nD < 0 || (p->nT && !p->t_samp) || (p->nV && !p->v_samp) || (p->nD && !p->d_samp))
            return set_err(FX_ERR_INVALID_ARGUMENT, "sampling ranges missing");
        if (p->nT > 4096 || p->nV > 4096 || p->nD > 4096) return set_err(FX_ERR_CAPACITY, "sampling range longer than 4096");
    }
    if (p->n_cost < 0 || p->n_cost > FX_NUM_COSTS) return set_err(FX_ERR_INVALID_ARGUMENT, "n_cost=%d", p->n_cost);
    if (p->lon_mode != FX_LON_VELOCITY_KEEPING && p->lon_mode != FX_LON_STOP_POINT)
        return set_err(FX_ERR_INVALID_ARGUMENT, "lon_mode=%d", p->lon_mode);
    if (p->lon_mode == FX_LON_STOP_POINT && p->sampling_matrix)
        return set_err(FX_ERR_INVALID_ARGUMENT, "stop-point sampling takes ranges, not a C x 13 matrix");
    for (int n = 0; n < p->n_cost; n++) {
        if (p->cost_id[n] < 0 || p->cost_id[n] >= FX_NUM_COSTS) return set_err(FX_ERR_INVALID_ARGUMENT, "unknown cost id %d", p->cost_id[n]);
        if (n && p->cost_id[n] <= p->cost_id[n - 1]) return set_err(FX_ERR_INVALID_ARGUMENT, "cost ids must be strictly ascending");
    }
    if (p->K > FX_MAX_OBSTACLES) return set_err(FX_ERR_CAPACITY, "at most %d obstacles per agent (K=%d)", FX_MAX_OBSTACLES, p->K);
    if (p->K < 0 || p->P < 0 || (p->K > 0 && (p->P < 2 || !p->obs_pos || !p->obs_cov_inv || !p->obs_npred)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "obstacle arrays inconsistent (K=%d, P=%d)", p->K, p->P);
    if ((p->mode & FX_MODE_COLLISION) && p->K > 0 && (!p->obs_hull || !p->obs_nhull))
        return set_err(FX_ERR_INVALID_ARGUMENT, "collision stage requested without obstacle hulls");
    if (p->n_dto < 0 || (p->n_dto > 0 && !p->dto_pos)) return set_err(FX_ERR_INVALID_ARGUMENT, "dto_pos missing");
    if (p->n_lane < 0 || (p->n_lane > 0 && (!p->lane_bbox || !p->lane_poly_off || !p->lane_poly || !p->lane_ctr_off || !p->lane_ctr)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "lanelet arrays missing (n_lane=%d)", p->n_lane);
    for (int l = 0; l < p->n_lane; l++)
        if (p->lane_poly_off[l + 1] < p->lane_poly_off[l] || p->lane_ctr_off[l + 1] < p->lane_ctr_off[l] || p->lane_poly_off[0] != 0 ||
            p->lane_ctr_off[0] != 0)
            return set_err(FX_ERR_INVALID_ARGUMENT, "lanelet offsets not ascending from 0 at lanelet %d", l);
    if (p->n_bound < 0 || (p->n_bound > 0 && (!p->bound_piece || !p->bound_bin || !p->bound_item)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "road boundary arrays missing (n_bound=%d)", p->n_bound);
    if ((p->mode & FX_MODE_ROAD_BOUNDARY) && p->n_bound > 0) {
        if (p->bound_bin[0] != 0) return set_err(FX_ERR_INVALID_ARGUMENT, "bound_bin[0] must be 0");
        for (int k = 0; k < p->M; k++)
            if (p->bound_bin[k + 1] < p->bound_bin[k]) return set_err(FX_ERR_INVALID_ARGUMENT, "bound_bin not ascending at %d", k);
        const int32_t n_item = p->bound_bin[p->M];
        for (int32_t j = 0; j < n_item; j++)
            if (p->bound_item[j] < 0 || p->bound_item[j] >= p->n_bound)
                return set_err(FX_ERR_INVALID_ARGUMENT, "bound_item[%d]=%d out of range", j, p->bound_item[j]);
        if (!(p->bound_d_reach > 0.0)) return set_err(FX_ERR_INVALID_ARGUMENT, "bound_d_reach must be positive");
    }
    return FX_OK;
}


// Step-major obstacle tables of one agent: rec[S][K][12] (mu, inverse covariance of prediction i-1; hull i-2), the per-step
// masks, and the hot table hot[S][K][FX_HOT_STRIDE] in the form the walk consumes (fx_walk.h, ObsHot).  Returns the margin of
// the broad phase's expanded circle test.
inline double pack_obstacle_tables(int S, int K, int P, const double *obs_pos, const double *obs_cov_inv, const int32_t *obs_npred,
                            const double *obs_hull, const int32_t *obs_nhull, bool have_hull, double ox, double oy,
                            double *rec, unsigned long long *pm, unsigned long long *hm, double *hot) {
    double r2_max = 0.0;
    for (int i = 0; i < S * mask_words(K); i++) pm[i] = hm[i] = 0ULL;
    for (int i = 0; i < S; i++) {
        for (int k = 0; k < K; k++) {
            const size_t mw = (size_t)(k >> 6) * S + i;   // word-major masks
            const unsigned long long mbit = 1ULL << (k & 63);
            double *q = rec + ((size_t)i * K + k) * 12;
            for (int e = 0; e < 12; e++) q[e] = 0.0;
            double *h = hot + ((size_t)i * K + k) * FX_HOT_STRIDE;
            for (int e = 0; e < FX_HOT_STRIDE; e++) h[e] = 0.0;
            if (i >= 1 && i < obs_npred[k] && i - 1 < P) {
                const double *mu = obs_pos + ((size_t)k * P + (i - 1)) * 2;
                const double *iv = obs_cov_inv + ((size_t)k * P + (i - 1)) * 4;
                q[0] = mu[0]; q[1] = mu[1]; q[2] = iv[0]; q[3] = iv[1]; q[4] = iv[2]; q[5] = iv[3];
                pm[mw] |= mbit;
                // Cholesky factor of the symmetric part of the inverse covariance: A = L^T L, L = [[l11, l12], [0, l22]];
                // the quadratic form r0 e0 + r1 e1 of the reference only sees that symmetric part.  No factor (not
                // positive definite, not finite): the entry stays zero, the form evaluates to 0 and the kernel redoes the
                // step from `rec`.
                const double a = iv[0], b = 0.5 * (iv[1] + iv[2]), dd = iv[3];
                const double l11 = std::sqrt(a), l12 = b / l11, l22sq = dd - l12 * l12;
                if (a > 0.0 && l22sq > 0.0 && std::isfinite(l11) && std::isfinite(l12) && std::isfinite(l22sq)) {
                    const double l22 = std::sqrt(l22sq), mx = mu[0] - ox, my = mu[1] - oy;
                    h[0] = l11; h[1] = l12; h[2] = l11 * mx + l12 * my; h[3] = l22; h[4] = l22 * my;
                }
            }
            if (have_hull && i >= 2 && i - 2 < obs_nhull[k]) {
                const double *oh = obs_hull + ((size_t)k * (P - 1) + (i - 2)) * 6;
                for (int e = 0; e < 6; e++) q[6 + e] = oh[e];
                hm[mw] |= mbit;
                // broad phase: circle that holds the hull (radius h1 + h2, with slack) in expanded form
                const double hx = oh[0] - ox, hy = oh[1] - oy, hr = (oh[4] + oh[5]) * 1.000001;
                h[5] = -2.0 * hx; h[6] = -2.0 * hy; h[7] = -2.0 * hr; h[8] = hx * hx + hy * hy - hr * hr;
                r2_max = std::max(r2_max, hx * hx + hy * hy);
            }
        }
    }
    // centre-gap values up to this margin go to the exact axis test: covers the rounding of the expanded form for ego hulls
    // within ~1 km of the origin (the pairs it adds are decided exactly, so decisions do not move)
    return 1e-6 + 4e-15 * (r2_max + 1e6);
}

// origin of the hot table's coordinates: the reference knot at the ego's arc length (any point near the ego does; it only
// keeps the products of the transformed forms small against their differences).  knots = [M][FX_REF_FIELDS] AoS.
inline void hot_origin_of(const double *knots, int M, double s0, double *origin) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (knots[(size_t)mid * FX_REF_FIELDS] > s0) hi = mid; else lo = mid + 1;
    }
    const int ko = std::min(std::max(lo - 1, 0), M - 1);
    origin[0] = knots[(size_t)ko * FX_REF_FIELDS + 4];
    origin[1] = knots[(size_t)ko * FX_REF_FIELDS + 5];
}

// Host writes into device memory (large BAR) -- OPT-IN (FX_STAGE=bar).  On boxes where the whole VRAM is mapped into the process a
// state update needs no staging launch: the host copies the rewritten range of its pinned block into the device arena itself --
// posted PCIe writes, ~50 GB/s and no round trip (tools/micro/bar_write.hip, bar_bw.hip; ~3 us of a host-fed step).  Round 5 ran it
// by default; it is opt-in now because two links of the chain are not a documented contract of HIP: (a) the writes pass through the
// host data path (HDP) of the GPU, which the driver flushes behind ITS OWN writes to VRAM -- the library now does the same: it reads
// the device's HDP flush register address (hipDeviceAttributeHdpMemFlushCntl), writes 1 behind the stores and reads it back; without
// that attribute the path is refused -- and (b) a kernel must not find a stale copy of a rewritten line in an XCD's L2: kernel start
// invalidates the L2s on gfx942 / gfx950, and the probe below checks exactly that (write, kernel reads every line, write again,
// kernel reads again), failing closed to the staging kernel.  The default path -- staging kernel reading the pinned block, DMA above
// 1 MiB -- is stream-ordered and needs neither.
// The probe cannot fault: the mapping is tested through a system call (read(2) into the address returns EFAULT where nothing is
// mapped), then patterns written by the host are read by a device-to-host copy AND by a kernel launch, twice with different
// contents (the second read finds the first pattern's lines in whatever cache kept them).
inline bool probe_host_writes(FxContext *c, int device, char *d_in, size_t bytes) {
    int large = 0;
    if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, device) != hipSuccess || !large || bytes < 64) return false;
    uint32_t *flush = nullptr;
    if (hipDeviceGetAttribute(reinterpret_cast<int *>(&flush), hipDeviceAttributeHdpMemFlushCntl, device) != hipSuccess || !flush) {
        (void)hipGetLastError();
        return false;
    }
    const int fd = open("/dev/zero", O_RDONLY);
    if (fd < 0) return false;
    char *first = d_in, *last = d_in + ((bytes - 64) & ~(size_t)63);
    const bool mapped = read(fd, first, 64) == 64 && read(fd, last, 64) == 64;
    close(fd);
    if (!mapped) return false;
    c->hdp_flush = flush;
    // a kernel reads what the host wrote: 64 workgroups (all XCDs) copy the probed line into a scratch buffer, which a plain copy
    // brings back; three rounds with different patterns over the SAME lines
    constexpr int kProbeBlocks = 64;
    FxDeviceBlock scratch;
    if (scratch.alloc(64 * kProbeBlocks)) { (void)hipGetLastError(); return false; }
    bool ok = true;
    unsigned long long pat[8], back[8];
    std::vector<unsigned long long> seen(8 * kProbeBlocks);
    for (int round = 0; round < 3 && ok; round++)
        for (char *at : {first, last}) {
            for (int i = 0; i < 8; i++)
                pat[i] = 0x9e3779b97f4a7c15ULL * (unsigned long long)(i + 1 + 8 * round) ^ (unsigned long long)(uintptr_t)at;
            memcpy(at, pat, sizeof(pat));
            __builtin_ia32_sfence();
            *c->hdp_flush = 1u; (void)*c->hdp_flush;
            ok = ok && fx_launch_probe_read(at, scratch.get(), kProbeBlocks, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess &&
                 hipMemcpy(seen.data(), scratch, 64 * kProbeBlocks, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(back, at, sizeof(back), hipMemcpyDeviceToHost) == hipSuccess && !memcmp(pat, back, sizeof(pat));
            for (int b = 0; b < kProbeBlocks && ok; b++) ok = !memcmp(pat, seen.data() + 8 * b, sizeof(pat));
        }
    if (!ok) { (void)hipGetLastError(); c->hdp_flush = nullptr; }
    return ok;
}
// the rewritten range of the pinned block, copied by the host (bar_ok; the caller has made sure the context's stream is idle)
inline void host_stage(FxContext *c, size_t lo, size_t hi) {
    memcpy(c->d_in + lo, c->h_in + lo, hi - lo);
    __builtin_ia32_sfence();
    *c->hdp_flush = 1u; (void)*c->hdp_flush;   // flush the GPU's host data path behind the stores (what the driver does behind its own)
    c->stage_path = 3;
}
// host writes only while NOTHING of this context's stream is pending: not the evaluation, not a top-k or publication kernel queued
// behind it, not work a caller put on a stream handed in with fx_set_stream -- any of them may still read the arena
inline bool host_stage_allowed(FxContext *c, size_t bytes) {
    // (hipStreamQuery is no help here: it reports hipErrorNotReady for a stream whose last kernel ended milliseconds ago until somebody
    // synchronises -- measured on ROCm 7.2 -- so the library keeps its own account of what may still read the arena)
    return c->bar_ok && !c->in_flight && !c->tail_work && bytes <= FX_STAGE_HOST_MAX;
}

inline int64_t max_candidates_of(const FxContext *c) {
    int64_t m = 0;
    for (int a = 0; a < c->n_agents; a++) m = std::max(m, c->slots[a].C);
    return m;
}
inline int check_agent(FxContext *c, int a) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "no evaluated plan step");
    if (a < 0 || a >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", a);
    return FX_OK;
}
