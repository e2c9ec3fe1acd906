// fx_api_sort.hip -- the stable cost order of all candidates of the last plan step, sorted on the device beside it and read back by
// rank (header: include/fxplan.h; kernels: fx_sort_kernel.h).  Nothing here runs in a plan step, and nothing a
// plan step, the top-k, a sparse set or the risk passes wrote or published is touched: the pass reads the cost and flag planes and
// writes its own block.  Behind it, the re-score of the last step under other cost weights, a pass of the same kind.
#include "fx_pass.h"
#include "fx_rescore_batch_plan.h"
#include "fx_rescore_plan.h"

extern "C" hipError_t fx_launch_sort(const FxSortArgs *args, int n_agents, int64_t max_C, hipEvent_t ev_start, hipEvent_t ev_stop,
                                     hipStream_t stream);
extern "C" hipError_t fx_launch_sort_gather(const int64_t *d_order, int64_t n, const double *cost, const uint32_t *flags, int64_t C,
                                            unsigned long long *out_cost, uint32_t *out_flags, hipStream_t stream);

#define FX_SORT_DEFINES_ONLY     // the sizes of fx_sort_kernel.h without its kernels (those are compiled in fx_kernels.hip)
#include "fx_sort_kernel.h"

struct FxSortOrder {
    long long step = -1;        // FxContext.n_steps when the agent was sorted: the next evaluation ends the order
    int64_t n_pool = 0, n_nan = 0;
};

struct FxSortState {
    explicit FxSortState(FxContext *c) : block(&c->dev_bytes) {}
    FxDeviceBlock block;        // every part 256-byte aligned (FxBlockLayout)
    int64_t total = 0;          // candidates (sum of the agents' leading dimensions) and tiles the layout below was made for
    int32_t tiles_max = 0, n_agents = 0;
    FxSortArgs args;            // device pointers into the block
    std::vector<FxSortAgent> agents;   // host copy of args.agents (uploaded when it changes: it must outlive the copy)
    bool agents_resident = false;      // the device holds `agents` as they are
    FxPinned<int64_t> h_counts;        // pinned + mapped [max_agents][2]: the kernels write n_pool, n_nan straight to the host
    std::vector<FxSortOrder> orders;   // [max_agents]
    FxEventPair ev;
};

void fx_sort_release(FxSortState *s) { delete s; }

static const FxSortOrder *valid_order(const FxContext *c, int agent) {
    if (!c->sort || agent < 0 || agent >= (int)c->sort->orders.size()) return nullptr;
    const FxSortOrder &o = c->sort->orders[agent];
    return (o.step == c->n_steps && fx_inputs_current(c)) ? &o : nullptr;
}

// sort agents [agent0, agent0 + n) of the last step; the callers have checked their arguments, everything else is checked here
// before this launches or writes
static int sort_agents(FxContext *c, int agent0, int n, uint32_t require, uint32_t exclude, int64_t *n_pool, int64_t *n_nan) {
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    if (!c->sort) {
        c->sort.reset(new FxSortState(c));
        c->sort->orders.resize((size_t)c->max_agents);
    }
    FxSortState *st = c->sort.get();
    const int A = c->n_agents;
    int64_t total = 0, max_all = 0, max_C = 0;
    for (int a = 0; a < A; a++) { total = std::max(total, c->slots[a].cand_off + c->slots[a].ld); max_all = std::max(max_all, c->slots[a].C); }
    for (int a = agent0; a < agent0 + n; a++) max_C = std::max(max_C, c->slots[a].C);
    const int32_t tiles_max = (int32_t)((max_all + FX_SORT_TILE - 1) / FX_SORT_TILE);
    if ((uint64_t)max_all >= (1ull << 32)) return set_err(FX_ERR_CAPACITY, "%lld candidates: the order holds 32-bit local indices", (long long)max_all);

    HIP_TRY(hipSetDevice(c->device));
    if (!st->h_counts) {
        FX_TRY(st->h_counts.alloc(2 * (size_t)c->max_agents, hipHostMallocMapped));
        st->args.counts = st->h_counts.dev;
    }
    if (total != st->total || tiles_max != st->tiles_max || A != st->n_agents || !st->block) {
        // another upload: a new layout, and no order of the old one is left
        FxBlockLayout lay;
        const size_t o_order = lay.take(sizeof(int64_t) * total), o_k0 = lay.take(sizeof(uint64_t) * total), o_k1 = lay.take(sizeof(uint64_t) * total);
        const size_t o_i0 = lay.take(sizeof(uint32_t) * total), o_i1 = lay.take(sizeof(uint32_t) * total);
        const size_t o_hist = lay.take(sizeof(uint32_t) * 256 * (size_t)tiles_max * A), o_dbase = lay.take(sizeof(uint32_t) * 256 * A);
        const size_t o_tc = lay.take(sizeof(uint32_t) * 2 * (size_t)tiles_max * A);
        const size_t o_ag = lay.take(sizeof(FxSortAgent) * A);
        for (FxSortOrder &o : st->orders) o.step = -1;
        // (a block that grows is freed: what was queued on it runs out first; tail_work stays as it is)
        if (lay.size() > st->block.size() && st->block) HIP_TRY(hipStreamSynchronize(c->stream));
        FX_TRY(st->block.ensure(lay.size()));
        char *b = st->block;
        FxSortArgs &g = st->args;
        g.order = reinterpret_cast<int64_t *>(b + o_order);
        g.key[0] = reinterpret_cast<unsigned long long *>(b + o_k0); g.key[1] = reinterpret_cast<unsigned long long *>(b + o_k1);
        g.idx[0] = reinterpret_cast<uint32_t *>(b + o_i0); g.idx[1] = reinterpret_cast<uint32_t *>(b + o_i1);
        g.hist = reinterpret_cast<uint32_t *>(b + o_hist); g.dbase = reinterpret_cast<uint32_t *>(b + o_dbase);
        g.tcount = reinterpret_cast<uint32_t *>(b + o_tc);
        g.agents = reinterpret_cast<const FxSortAgent *>(b + o_ag);
        st->total = total; st->tiles_max = tiles_max; st->n_agents = A;
        st->agents.assign((size_t)A, FxSortAgent{nullptr, nullptr, 0, 0});
        st->agents_resident = false;
    }
    bool same = st->agents_resident;
    for (int a = 0; a < A; a++) {
        const FxAgentSlot &sl = c->slots[a];
        const FxSortAgent &h = st->agents[a];
        same = same && h.cost == c->d_cost + sl.cand_off && h.flags == c->d_flags + sl.cand_off && h.C == sl.C && h.off == sl.cand_off;
    }
    if (!same) {
        // (an earlier upload came from this host vector: it has landed before the vector is rewritten)
        FX_TRY(fx_drain(c));
        for (int a = 0; a < A; a++) {
            const FxAgentSlot &sl = c->slots[a];
            st->agents[a] = FxSortAgent{c->d_cost + sl.cand_off, c->d_flags + sl.cand_off, sl.C, sl.cand_off};
        }
        st->agents_resident = false;
    }
    FxSortArgs g = st->args;
    g.require = require; g.exclude = exclude; g.agent0 = agent0; g.tiles_max = tiles_max;
    for (int a = agent0; a < agent0 + n; a++) st->orders[a].step = -1;   // from here on the previous orders of these agents are gone
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    if (!st->agents_resident) {
        HIP_TRY(hipMemcpyAsync(const_cast<FxSortAgent *>(g.agents), st->agents.data(), sizeof(FxSortAgent) * A, hipMemcpyHostToDevice, c->stream));
        st->agents_resident = true;
    }
    for (int a = agent0; a < agent0 + n; a++) st->h_counts[2 * a] = st->h_counts[2 * a + 1] = -1;   // (the stream is idle or behind a kernel boundary)
    HIP_TRY(fx_launch_sort(&g, n, max_C, st->ev.e0, st->ev.e1, c->stream));
    st->ev.timed = true;
    c->in_flight = true; c->tail_work = true;
    FX_TRY(fx_drain(c));
    for (int a = agent0; a < agent0 + n; a++) {
        FxSortOrder &o = st->orders[a];
        o.n_pool = st->h_counts[2 * a]; o.n_nan = st->h_counts[2 * a + 1];
        if (o.n_pool < 0 || o.n_pool > c->slots[a].C || o.n_nan < 0 || o.n_nan > o.n_pool)
            return set_err(FX_ERR_HIP, "the sort of agent %d reported %lld pool members, %lld NaNs of %lld candidates", a, (long long)o.n_pool,
                           (long long)o.n_nan, (long long)c->slots[a].C);
        o.step = c->n_steps;
        if (n_pool) n_pool[a - agent0] = o.n_pool;
        if (n_nan) n_nan[a - agent0] = o.n_nan;
    }
    return FX_OK;
}

extern "C" {

int32_t fx_sort_candidates_agent(FxContext *c, int32_t agent, uint32_t require, uint32_t exclude, int64_t *n_pool, int64_t *n_nan) {
    FX_TRY(check_agent(c, agent));
    if (!n_pool || !n_nan) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_sort_candidates_agent: NULL argument");
    return sort_agents(c, agent, 1, require, exclude, n_pool, n_nan);
}

int32_t fx_sort_candidates_batch(FxContext *c, uint32_t require, uint32_t exclude, int64_t *n_pool, int64_t *n_nan) {
    FX_TRY(check_agent(c, 0));
    if (!n_pool || !n_nan) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_sort_candidates_batch: NULL argument");
    return sort_agents(c, 0, c->n_agents, require, exclude, n_pool, n_nan);
}

int32_t fx_read_ranked_agent(FxContext *c, int32_t agent, int64_t first, int64_t n, int64_t *index, double *cost, uint32_t *flags) {
    FX_TRY(check_agent(c, agent));
    const FxSortOrder *o = valid_order(c, agent);
    if (!o) return set_err(FX_ERR_NOT_READY, "agent %d has no valid order (fx_sort_candidates_agent since the last evaluation)", agent);
    if (first < 0 || n < 0 || first > o->n_pool || n > o->n_pool - first)
        return set_err(FX_ERR_INVALID_ARGUMENT, "ranks [%lld, %lld + %lld) outside the pool of %lld", (long long)first, (long long)first,
                       (long long)n, (long long)o->n_pool);
    if (n > 0 && !index) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_read_ranked_agent: index is NULL");
    if (n == 0) return FX_OK;
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    const FxSortState *st = c->sort.get();
    const FxAgentSlot &sl = c->slots[agent];
    const int64_t *d_order = st->args.order + sl.cand_off + first;
    HIP_TRY(hipSetDevice(c->device));
    if (cost || flags) {
        // gathered into the agent's segment of the first key / index buffers, which only a sort writes (same stream, behind this)
        unsigned long long *g_cost = st->args.key[0] + sl.cand_off;
        uint32_t *g_flags = st->args.idx[0] + sl.cand_off;
        HIP_TRY(fx_launch_sort_gather(d_order, n, c->d_cost + sl.cand_off, c->d_flags + sl.cand_off, sl.C, cost ? g_cost : nullptr,
                                      flags ? g_flags : nullptr, c->stream));
        c->in_flight = true; c->tail_work = true;
        FX_TRY(fx_drain(c));
        if (cost) HIP_TRY(hipMemcpy(cost, g_cost, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (flags) HIP_TRY(hipMemcpy(flags, g_flags, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    } else {
        FX_TRY(fx_drain(c));
    }
    HIP_TRY(hipMemcpy(index, d_order, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    return FX_OK;
}

int32_t fx_sort_views(FxContext *c, int32_t agent, void **d_index, int64_t *n_pool) {
    FX_TRY(check_agent(c, agent));
    if (!d_index) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_sort_views: d_index is NULL");
    const FxSortOrder *o = valid_order(c, agent);
    if (!o) return set_err(FX_ERR_NOT_READY, "agent %d has no valid order (fx_sort_candidates_agent since the last evaluation)", agent);
    *d_index = c->sort->args.order + c->slots[agent].cand_off;
    if (n_pool) *n_pool = o->n_pool;
    return FX_OK;
}

// device time of the context's last sort (events around its launch sequence), ms; -1 before the first
double fx_last_sort_ms(FxContext *c) { return (c && c->sort) ? c->sort->ev.elapsed_ms() : -1.0; }

}  // extern "C"

// ---- the last plan step re-scored under many cost-weight vectors at once (kernels: fx_rescore_kernel.h; launch
// rule: fx_rescore_plan.h).  Like the sort it reads planes of the step -- the raw cost rows and the flag words -- and writes a block of
// its own. ----
// (weak: a host-only program that links these files against launcher stubs of its own need not define it)
extern "C" __attribute__((weak)) hipError_t fx_launch_rescore(const FxRescoreArgs *a, const FxRescorePlan *p, hipEvent_t ev_start,
                                                              hipEvent_t ev_stop, hipStream_t stream);
extern "C" __attribute__((weak)) hipError_t fx_launch_rescore_batch(const FxRescoreBatchArgs *a, hipEvent_t ev_start, hipEvent_t ev_stop,
                                                                    hipStream_t stream);

struct FxRescoreState {
    explicit FxRescoreState(FxContext *c) : block(&c->dev_bytes) {}
    FxDeviceBlock block;   // staged weights | partials | winners | costs | totals, every part 256-byte aligned (FxBlockLayout); the table
                           // calls below lay it out as staging | partials | winners and costs | totals
    FxEventPair ev;
    // the table calls (fx_rescore_agent_rows, fx_rescore_batch): what goes up in one copy -- descriptors | offsets | weights |
    // external rows -- and the winners and costs that come back in one; pinned, grow-only
    FxPinned<char> up, down;
};

void fx_rescore_release(FxRescoreState *s) { delete s; }

// (launcher hook of the tests and of tools/bench_rescore.py, not part of fxplan.h: 0 the rule of fx_rescore_plan, FX_RESCORE_LANE /
// FX_RESCORE_VECTOR that regime whatever the number of vectors -- the results do not depend on it)
static std::atomic<int> fx_rescore_regime_forced{0};

extern "C" {

void fx_rescore_set_regime(int32_t regime) {
    fx_rescore_regime_forced.store((regime == FX_RESCORE_LANE || regime == FX_RESCORE_VECTOR) ? regime : 0, std::memory_order_relaxed);
}
// the regime a call of n candidates and n_vec vectors takes
int32_t fx_rescore_regime(int64_t n, int32_t n_vec) {
    return fx_rescore_plan(n, n_vec, fx_rescore_regime_forced.load(std::memory_order_relaxed)).regime;
}

int32_t fx_device_costmap_view(FxContext *c, int32_t agent, void **costmap, int64_t *ld, int32_t *n_cost) {
    FX_TRY(check_agent(c, agent));
    const FxAgentSlot &s = c->slots[agent];
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_COSTMAP");
    if (costmap) *costmap = c->d_costmap + (size_t)FX_NUM_COSTS * s.cand_off;
    if (ld) *ld = s.ld;
    if (n_cost) *n_cost = s.n_cost;
    return FX_OK;
}

int32_t fx_rescore_agent(FxContext *c, int32_t agent, int32_t n_vec, const double *w, int64_t *winner, double *cost, double *totals) {
    // every refusal stands in front of the first allocation, copy or launch
    FX_TRY(check_agent(c, agent));
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    const FxAgentSlot &s = c->slots[agent];
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_COSTMAP");
    if (n_vec < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_agent: n_vec %d", n_vec);
    if (!w || !winner || !cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_agent: NULL argument");
    if (n_vec > FX_RESCORE_MAX_VECTORS) return set_err(FX_ERR_CAPACITY, "%d weight vectors: at most %d per call", n_vec, FX_RESCORE_MAX_VECTORS);
    const DevProblem &hp = c->h_probs[agent];
    const int n_cost = hp.n_cost;
    for (size_t k = 0; k < (size_t)n_vec * n_cost; k++)
        if (!(w[k] != 0.0) || !std::isfinite(w[k]))
            return set_err(FX_ERR_INVALID_ARGUMENT, "weight %d of vector %lld is %g: weights are finite and not zero (a zero weight is another cost list)",
                           (int)(k % n_cost), (long long)(k / n_cost), w[k]);
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    if (!fx_launch_rescore) return set_err(FX_ERR_HIP, "built without the re-score launcher");
    const FxRescorePlan plan = fx_rescore_plan(s.C, n_vec, fx_rescore_regime_forced.load(std::memory_order_relaxed));
    if (plan.n_part > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "%lld candidates: %lld workgroups", (long long)s.C, (long long)plan.n_part);

    HIP_TRY(hipSetDevice(c->device));
    if (!c->rescore) c->rescore.reset(new FxRescoreState(c));
    FxRescoreState *st = c->rescore.get();
    const size_t W = (size_t)n_vec, parts = fx_rescore_partials(plan, n_vec), n = (size_t)s.C;
    FxBlockLayout lay;
    const size_t o_w = lay.take(sizeof(double) * W * n_cost), o_pc = lay.take(sizeof(double) * parts), o_pi = lay.take(sizeof(long long) * parts);
    const size_t o_win = lay.take(sizeof(long long) * W), o_cost = lay.take(sizeof(double) * W);
    const size_t o_tot = totals ? lay.take(sizeof(double) * W * n) : 0;
    // (a block that grows is freed: what was queued on it runs out first)
    if (lay.size() > st->block.size() && st->block) HIP_TRY(hipStreamSynchronize(c->stream));
    FX_TRY(st->block.ensure(lay.size()));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block;

    FxRescoreArgs a{};
    a.costmap = c->d_costmap + (size_t)FX_NUM_COSTS * s.cand_off;
    a.flags = c->d_flags + s.cand_off;
    a.n = s.C, a.ld = s.ld, a.n_cost = n_cost, a.n_vec = n_vec;
    a.n_pred = -1;
    for (int m = 0; m < n_cost; m++)
        if (hp.cost_id[m] == FX_COST_PREDICTION) a.n_pred = m;
    // (a deferred step without a prediction term closed nothing in the obstacle kernel: its costs are the walk's own sums)
    a.deferred = ((hp.mode & FX_MODE_INT_DEFER_OBST) && a.n_pred >= 0) ? 1 : 0;
    a.w = reinterpret_cast<const double *>(b + o_w);
    a.part_cost = reinterpret_cast<double *>(b + o_pc), a.part_idx = reinterpret_cast<long long *>(b + o_pi);
    a.winner = reinterpret_cast<long long *>(b + o_win), a.cost = reinterpret_cast<double *>(b + o_cost);
    a.totals = totals ? reinterpret_cast<double *>(b + o_tot) : nullptr;
    c->in_flight = true; c->tail_work = true;
    if (n_cost > 0) HIP_TRY(hipMemcpyAsync(b + o_w, w, sizeof(double) * W * n_cost, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(fx_launch_rescore(&a, &plan, st->ev.e0, st->ev.e1, c->stream));
    st->ev.timed = true;
    static_assert(sizeof(long long) == sizeof(int64_t), "the winners are copied as they are");
    HIP_TRY(hipMemcpyAsync(winner, a.winner, sizeof(int64_t) * W, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(cost, a.cost, sizeof(double) * W, hipMemcpyDeviceToHost, c->stream));
    if (totals && n > 0) HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof(double) * W * n, hipMemcpyDeviceToHost, c->stream));
    return fx_drain(c);
}

// device time of the context's last re-score (events around its launches), ms; -1 before the first
double fx_last_rescore_ms(FxContext *c) { return (c && c->rescore) ? c->rescore->ev.elapsed_ms() : -1.0; }

}  // extern "C"

// ---- the re-score over EFFECTIVE cost lists and for several agents in one call (kernels:
// fx_rescore_batch_kernel.h; table: fx_rescore_batch_plan.h).  An agent's effective list is the step's own list with two optional rows
// from outside the step: pred [C] in place of the prediction's row, resp [C] one more term at fx_resp_term_at.  Both entry points
// run the one path below: checks, one staging buffer up, three launches at most, winners and costs back in one copy. ----
struct RescoreEntryCall {
    int32_t agent, n_vec, n_eff, n_pred, at;   // at: position of the responsibility term in the effective list, -1 without one
    const double *w, *pred, *resp;
};

// what fx_rescore_agent refuses, for one listed agent, and the effective list; who: "" or "agent 3: "
static int rescore_entry_check(FxContext *c, const char *who, RescoreEntryCall &q) {
    const FxAgentSlot &s = c->slots[q.agent];
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "%splan step ran without FX_MODE_WRITE_COSTMAP", who);
    if (q.n_vec < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "%sn_vec %d", who, q.n_vec);
    if (q.n_vec > FX_RESCORE_MAX_VECTORS)
        return set_err(FX_ERR_CAPACITY, "%s%d weight vectors: at most %d per agent", who, q.n_vec, FX_RESCORE_MAX_VECTORS);
    const DevProblem &hp = c->h_probs[q.agent];
    q.n_pred = -1;
    for (int m = 0; m < hp.n_cost; m++)
        if (hp.cost_id[m] == FX_COST_PREDICTION) q.n_pred = m;
    if (q.pred && q.n_pred < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "%sa prediction row for a cost list without a prediction term", who);
    q.at = q.resp ? fx_resp_term_at(hp.cost_id, hp.n_cost) : -1;
    q.n_eff = hp.n_cost + (q.resp ? 1 : 0);
    if (!q.w) return set_err(FX_ERR_INVALID_ARGUMENT, "%sthe weights are NULL", who);
    for (size_t k = 0; k < (size_t)q.n_vec * q.n_eff; k++)
        if (!(q.w[k] != 0.0) || !std::isfinite(q.w[k]))
            return set_err(FX_ERR_INVALID_ARGUMENT,
                           "%sweight %d of vector %lld is %g: weights are finite and not zero (a zero weight is another cost list)", who,
                           (int)(k % q.n_eff), (long long)(k / q.n_eff), q.w[k]);
    return FX_OK;
}

// the checked entries of a call; winner / cost [sum of n_vec] in call order; totals [n_vec][C] only for a call of one entry
static int rescore_entries(FxContext *c, const std::vector<RescoreEntryCall> &calls, int64_t *winner, double *cost, double *totals) {
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    if (!fx_launch_rescore_batch) return set_err(FX_ERR_HIP, "built without the batched re-score launcher");
    const int E = (int)calls.size(), forced = fx_rescore_regime_forced.load(std::memory_order_relaxed);
    std::vector<FxRescoreBatchItem> items((size_t)E);
    for (int i = 0; i < E; i++) items[i] = FxRescoreBatchItem{c->slots[calls[i].agent].C, calls[i].n_vec};
    FxRescoreBatchPlan t;
    int bad = 0;
    if (fx_rescore_batch_plan(items.data(), E, forced, t, &bad))   // (the vector counts were checked: what is left is a grid)
        return set_err(FX_ERR_CAPACITY, "agent %d: the call's flat grid exceeds %lld workgroups", calls[bad].agent, (long long)FX_RESCORE_GRID_MAX);
    // the totals of a vector-regime entry: one more table entry, the lane kernel without its reduction (as fx_launch_rescore)
    const bool tot_entry = totals && E == 1 && t.rows[0].plan.regime == FX_RESCORE_VECTOR && items[0].n > 0;
    FxRescorePlan tot_plan;
    if (tot_entry) {
        tot_plan = fx_rescore_plan(items[0].n, items[0].n_vec, FX_RESCORE_LANE);
        if (tot_plan.n_part * tot_plan.grid_y > FX_RESCORE_GRID_MAX)
            return set_err(FX_ERR_CAPACITY, "agent %d: the totals' grid exceeds %lld workgroups", calls[0].agent, (long long)FX_RESCORE_GRID_MAX);
    }

    HIP_TRY(hipSetDevice(c->device));
    if (!c->rescore) c->rescore.reset(new FxRescoreState(c));
    FxRescoreState *st = c->rescore.get();
    // what goes up: descriptors | offsets | weights | external rows
    FxBlockLayout up;
    const size_t n_desc = (size_t)E + (tot_entry ? 1 : 0);
    const size_t u_desc = up.take(sizeof(FxRescoreEntry) * n_desc), u_off = up.take(sizeof(int64_t) * (2 * (size_t)E + 1));
    std::vector<size_t> u_w((size_t)E), u_pred((size_t)E, 0), u_resp((size_t)E, 0);
    for (int i = 0; i < E; i++) {
        const size_t n = (size_t)items[i].n;
        u_w[i] = up.take(sizeof(double) * (size_t)calls[i].n_vec * calls[i].n_eff);
        if (calls[i].pred) u_pred[i] = up.take(sizeof(double) * n);
        if (calls[i].resp) u_resp[i] = up.take(sizeof(double) * n);
    }
    const size_t V = (size_t)t.vectors, parts = (size_t)t.partials;
    FxBlockLayout lay;
    const size_t o_up = lay.take(up.size()), o_pc = lay.take(sizeof(double) * parts), o_pi = lay.take(sizeof(long long) * parts);
    const size_t o_out = lay.take((sizeof(long long) + sizeof(double)) * V);   // winners, then costs: one part, one copy back
    const size_t o_tot = totals ? lay.take(sizeof(double) * (size_t)items[0].n_vec * (size_t)items[0].n) : 0;
    // (a block that grows is freed: what was queued on it runs out first)
    if (lay.size() > st->block.size() && st->block) HIP_TRY(hipStreamSynchronize(c->stream));
    FX_TRY(st->block.ensure(lay.size()));
    if (up.size() > st->up.size() || (sizeof(long long) + sizeof(double)) * V > st->down.size()) HIP_TRY(hipStreamSynchronize(c->stream));
    FX_TRY(st->up.ensure(up.size(), hipHostMallocDefault));
    FX_TRY(st->down.ensure((sizeof(long long) + sizeof(double)) * V, hipHostMallocDefault));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block, *h = st->up;
    char *d_up = b + o_up;
    long long *d_win = reinterpret_cast<long long *>(b + o_out);
    double *d_cost = reinterpret_cast<double *>(b + o_out + sizeof(long long) * V);

    FxRescoreEntry *desc = reinterpret_cast<FxRescoreEntry *>(h + u_desc);
    int64_t *off = reinterpret_cast<int64_t *>(h + u_off);
    for (int i = 0; i < E; i++) {
        const RescoreEntryCall &q = calls[i];
        const FxRescoreBatchRow &r = t.rows[i];
        const FxAgentSlot &s = c->slots[q.agent];
        const DevProblem &hp = c->h_probs[q.agent];
        const size_t n = (size_t)s.C;
        FxRescoreEntry e{};
        const double *costmap = c->d_costmap + (size_t)FX_NUM_COSTS * s.cand_off;
        int k = 0;
        for (int m = 0; m <= hp.n_cost; m++) {
            if (m == q.at) e.row[k++] = reinterpret_cast<const double *>(d_up + u_resp[i]);
            if (m == hp.n_cost) break;
            e.row[k++] = (m == q.n_pred && q.pred) ? reinterpret_cast<const double *>(d_up + u_pred[i]) : costmap + (size_t)m * s.ld;
        }
        e.flags = c->d_flags + s.cand_off;
        e.w = reinterpret_cast<const double *>(d_up + u_w[i]);
        e.part_cost = reinterpret_cast<double *>(b + o_pc) + r.part0, e.part_idx = reinterpret_cast<long long *>(b + o_pi) + r.part0;
        e.winner = d_win + r.out0, e.cost = d_cost + r.out0;
        e.totals = (totals && r.plan.regime == FX_RESCORE_LANE) ? reinterpret_cast<double *>(b + o_tot) : nullptr;
        e.n = s.C, e.n_part = r.plan.n_part, e.per = r.plan.per;
        e.wg0 = r.wg0, e.fin0 = r.fin0;
        e.n_cost = q.n_eff, e.n_pred = q.n_pred;   // (the responsibility term stands behind the prediction: its position stays)
        // (a deferred step without a prediction term closed nothing in the obstacle kernel: its costs are the walk's own sums)
        e.deferred = ((hp.mode & FX_MODE_INT_DEFER_OBST) && q.n_pred >= 0) ? 1 : 0;
        e.n_vec = q.n_vec, e.vec_chunk = r.plan.vec_chunk;
        desc[r.slot] = e;
        off[r.slot] = r.wg0, off[E + r.slot] = r.fin0;
        memcpy(h + u_w[i], q.w, sizeof(double) * (size_t)q.n_vec * q.n_eff);
        if (q.pred && n > 0) memcpy(h + u_pred[i], q.pred, sizeof(double) * n);
        if (q.resp && n > 0) memcpy(h + u_resp[i], q.resp, sizeof(double) * n);
    }
    FxRescoreBatchArgs a{};
    a.entries = reinterpret_cast<const FxRescoreEntry *>(d_up + u_desc);
    a.wg0 = reinterpret_cast<const int64_t *>(d_up + u_off);
    a.n_lane = t.n_lane, a.n_vector = t.n_vector;
    a.lane_wgs = t.lane_wgs, a.vector_wgs = t.vector_wgs, a.finish_blocks = t.finish_blocks, a.n_waves = t.vectors;
    if (tot_entry) {
        FxRescoreEntry e = desc[0];
        e.totals = reinterpret_cast<double *>(b + o_tot);
        e.part_cost = nullptr, e.part_idx = nullptr;
        e.n_part = tot_plan.n_part, e.per = tot_plan.per, e.vec_chunk = tot_plan.vec_chunk, e.wg0 = 0;
        desc[E] = e;
        off[2 * E] = 0;
        a.tot_entries = a.entries + E, a.tot_wg0 = a.wg0 + 2 * E, a.n_tot = 1, a.tot_wgs = tot_plan.n_part * tot_plan.grid_y;
    }
    c->in_flight = true; c->tail_work = true;
    HIP_TRY(hipMemcpyAsync(d_up, h, up.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(fx_launch_rescore_batch(&a, st->ev.e0, st->ev.e1, c->stream));
    st->ev.timed = true;
    static_assert(sizeof(long long) == sizeof(int64_t), "the winners are copied as they are");
    HIP_TRY(hipMemcpyAsync(st->down.get(), b + o_out, (sizeof(long long) + sizeof(double)) * V, hipMemcpyDeviceToHost, c->stream));
    if (totals && items[0].n > 0)
        HIP_TRY(hipMemcpyAsync(totals, b + o_tot, sizeof(double) * (size_t)items[0].n_vec * (size_t)items[0].n, hipMemcpyDeviceToHost, c->stream));
    FX_TRY(fx_drain(c));
    memcpy(winner, st->down.get(), sizeof(int64_t) * V);
    memcpy(cost, st->down.get() + sizeof(long long) * V, sizeof(double) * V);
    return FX_OK;
}

extern "C" {

int32_t fx_rescore_agent_rows(FxContext *c, int32_t agent, int32_t n_vec, const double *w, const double *pred, const double *resp,
                              int64_t *winner, double *cost, double *totals) {
    // every refusal stands in front of the first allocation, copy or launch
    FX_TRY(check_agent(c, agent));
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    if (!w || !winner || !cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_agent_rows: NULL argument");
    std::vector<RescoreEntryCall> calls(1, RescoreEntryCall{agent, n_vec, 0, -1, -1, w, pred, resp});
    FX_TRY(rescore_entry_check(c, "", calls[0]));
    return rescore_entries(c, calls, winner, cost, totals);
}

int32_t fx_rescore_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const int32_t *n_vec, const double *w,
                         const double *const *pred, const double *const *resp, int64_t *winner, double *cost) {
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_batch: n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;   // (no agent: nothing is touched, the context included)
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!n_vec || !w || !winner || !cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_batch: NULL argument");
    FX_TRY(check_agent(c, 0));
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    std::vector<RescoreEntryCall> calls((size_t)n_agents);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (int i = 0; i < n_agents; i++) {
        const int32_t agent = agents ? agents[i] : i;
        if (agent < 0 || agent >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
        if (listed[agent]++) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        calls[i] = RescoreEntryCall{agent, n_vec[i], 0, -1, -1, w, pred ? pred[i] : nullptr, resp ? resp[i] : nullptr};
        char who[32];
        snprintf(who, sizeof(who), "agent %d: ", agent);
        FX_TRY(rescore_entry_check(c, who, calls[i]));
        w += (size_t)calls[i].n_vec * calls[i].n_eff;
    }
    return rescore_entries(c, calls, winner, cost, nullptr);
}

}  // extern "C"

// ---- the obstacle stage of the last plan step run again over many prediction sets at once (kernels:
// fx_hypotheses_kernel.h; rounds: fx_hypotheses_plan.h).  Like the re-score it reads planes of the step -- x, y, theta, the raw cost rows,
// the flag words -- and writes a block of its own. ----
#include "fx_hypotheses_plan.h"

// (weak: a host-only program that links these files against launcher stubs of its own need not define it)
extern "C" __attribute__((weak)) hipError_t fx_launch_hypotheses(const FxHypArgs *a, size_t lds_bytes, hipStream_t stream);

static_assert(FX_HYP_MAX == FX_HYPOTHESES_MAX, "fxplan.h states the limit of fx_hypotheses_plan.h");

struct FxHypState {
    explicit FxHypState(FxContext *c) : block(&c->dev_bytes) {}
    FxDeviceBlock block;   // tables of the call | what comes back (answers, then the rows asked for) | a round's scratch, laid out by FxBlockLayout
    FxEventPair ev;
    FxPinned<char> up, down;   // the tables' staging buffer; everything that comes back, in one copy.  Grow-only
    int32_t CH = 0, rounds = 0, launches = 0;   // of the last call (fx_last_hypotheses_info)
    bool called = false;
};

void fx_hyp_release(FxHypState *s) { delete s; }

// (hook of the tests and of tools/bench_hypotheses.py, not part of fxplan.h: bytes of tables plus scratch per round, 0 = FX_ITEM_SCRATCH_BYTES)
static std::atomic<size_t> fx_hyp_scratch_limit{0};

extern "C" {

void fx_hypotheses_set_scratch_limit(size_t bytes) { fx_hyp_scratch_limit.store(bytes, std::memory_order_relaxed); }

int32_t fx_eval_hypotheses_agent(FxContext *c, int32_t agent, int32_t n_hyp, const FxHypothesis *hyp, const FxHypothesisOutputs *out) {
    // every refusal stands in front of the first allocation, copy or launch
    FX_TRY(check_agent(c, agent));
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
    const FxAgentSlot &s = c->slots[agent];
    const DevProblem &hp = c->h_probs[agent];
    if (!(s.mode & FX_MODE_WRITE_BUNDLE)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_BUNDLE");
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "plan step ran without FX_MODE_WRITE_COSTMAP");
    if (n_hyp < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_eval_hypotheses_agent: n_hyp %d", n_hyp);
    if (!hyp || !out || !out->winner || !out->cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_eval_hypotheses_agent: NULL argument");
    if (s.K <= 0) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d was uploaded without obstacles (K = 0): upload again", agent);
    bool windowed = false;
    for (int m = 0; m < hp.n_cost; m++) windowed |= fx_is_windowed_cost(hp.cost_id[m]);
    // (K <= 64 is also what the tables and the kernels are sized for: one mask word per step, obstacle k on lane k of the cull)
    if (s.K > 64 || (hp.mode & FX_MODE_ROAD_BOUNDARY) || windowed)
        return set_err(FX_ERR_INVALID_ARGUMENT, "the obstacle kernel is not applicable to this step (needs FX_MODE_WRITE_BUNDLE, K <= 64, no road "
                       "boundary, no windowed cost term)");
    if (n_hyp > FX_HYP_MAX) return set_err(FX_ERR_CAPACITY, "%d hypotheses: at most %d per call", n_hyp, FX_HYP_MAX);
    for (int h = 0; h < n_hyp; h++)
        if (!hyp[h].obs_pos || !hyp[h].obs_cov_inv || !hyp[h].obs_npred || !hyp[h].obs_hull || !hyp[h].obs_nhull)
            return set_err(FX_ERR_INVALID_ARGUMENT, "hypothesis %d: a NULL array (an absent obstacle has obs_npred = 0 and obs_nhull = 0)", h);
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    if (!fx_launch_hypotheses) return set_err(FX_ERR_HIP, "built without the hypotheses launcher");
    const int S = hp.S, K = s.K, P = s.P, CH = c->plan.split_CH;
    const size_t limit_forced = fx_hyp_scratch_limit.load(std::memory_order_relaxed);
    FxHypPlan plan;
    if (!fx_hypotheses_plan(s.C, s.ld, S, K, CH, n_hyp, limit_forced ? limit_forced : FX_ITEM_SCRATCH_BYTES, plan))
        return set_err(FX_ERR_CAPACITY, "%lld candidates: %lld items per hypothesis", (long long)s.C, (long long)plan.items);

    HIP_TRY(hipSetDevice(c->device));
    if (!c->hyp) c->hyp.reset(new FxHypState(c));
    FxHypState *st = c->hyp.get();
    const size_t H = (size_t)n_hyp, R = (size_t)plan.per_round, n = (size_t)s.C, ld = (size_t)s.ld, NC = (size_t)plan.NC;
    const FxHypTable T = fx_hyp_table(S, K);
    const size_t up_bytes = H * plan.table_words * 8;
    // what comes back, one part of the block and ONE copy: winners, counts, costs | pred | total | collision (the rows where asked
    // for), staged through the pinned `down` buffer
    FxBlockLayout back;
    const size_t k_ans = back.take(H * (2 * sizeof(long long) + sizeof(double)));
    const size_t k_pred = out->pred ? back.take(sizeof(double) * H * n) : 0, k_total = out->total ? back.take(sizeof(double) * H * n) : 0;
    const size_t k_col = out->collision ? back.take(H * n) : 0;
    const size_t down_bytes = back.size();
    FxBlockLayout lay;
    const size_t o_tab = lay.take(up_bytes), o_back = lay.take(down_bytes);
    const size_t o_out = o_back + k_ans, o_pred = o_back + k_pred, o_total = o_back + k_total, o_col = o_back + k_col;
    const size_t o_part = lay.take(sizeof(double) * R * NC * ld), o_colm = lay.take(8 * R * NC * (size_t)plan.n_tiles);
    const size_t o_tot = lay.take(sizeof(double) * R * ld), o_colb = lay.take(R * ld);
    const size_t o_pc = lay.take(sizeof(double) * R * (size_t)plan.n_part), o_pi = lay.take(sizeof(long long) * R * (size_t)plan.n_part);
    // (a block that grows is freed: what was queued on it runs out first)
    if ((lay.size() > st->block.size() && st->block) || up_bytes > st->up.size() || down_bytes > st->down.size())
        HIP_TRY(hipStreamSynchronize(c->stream));
    FX_TRY(st->block.ensure(lay.size()));
    FX_TRY(st->up.ensure(up_bytes, hipHostMallocDefault));
    FX_TRY(st->down.ensure(down_bytes, hipHostMallocDefault));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block;

    // one table per hypothesis, packed as a state update packs the step's (the step's hot_origin), into one staging buffer
    for (size_t h = 0; h < H; h++) {
        double *t = reinterpret_cast<double *>(st->up.get()) + h * plan.table_words;
        t[T.margin] = pack_obstacle_tables(S, K, P, hyp[h].obs_pos, hyp[h].obs_cov_inv, hyp[h].obs_npred, hyp[h].obs_hull, hyp[h].obs_nhull,
                                           s.have_hull, hp.hot_origin[0], hp.hot_origin[1], t + T.rec,
                                           reinterpret_cast<unsigned long long *>(t + T.pm), reinterpret_cast<unsigned long long *>(t + T.hm), t + T.hot);
    }
    FxHypArgs a{};
    a.planes = hp.planes, a.flags = hp.flags, a.costmap = hp.costmap;
    a.C = s.C, a.ld = s.ld, a.S = S, a.K = K;
    a.n_cost = hp.n_cost, a.n_pred = -1;
    for (int m = 0; m < hp.n_cost; m++) {
        a.w[m] = hp.cost_w[m];
        if (hp.cost_id[m] == FX_COST_PREDICTION) a.n_pred = m;
    }
    a.deferred = a.n_pred >= 0 ? 1 : 0;   // (without a prediction term the obstacle kernel closes nothing: the walk's own sum)
    a.col_mode = ((hp.mode & FX_MODE_COLLISION) && s.have_hull) ? 1 : 0;
    a.ox = hp.hot_origin[0], a.oy = hp.hot_origin[1];
    a.wb = hp.veh.wb_rear_axle, a.half_len = hp.veh.length / 2, a.half_wid = hp.veh.width / 2;
    a.table_words = plan.table_words, a.CH = plan.CH, a.NC = plan.NC, a.n_tiles = plan.n_tiles, a.n_part = plan.n_part;
    a.part = reinterpret_cast<double *>(b + o_part), a.colm = reinterpret_cast<unsigned long long *>(b + o_colm);
    a.tot = reinterpret_cast<double *>(b + o_tot), a.colb = reinterpret_cast<unsigned char *>(b + o_colb);
    a.part_cost = reinterpret_cast<double *>(b + o_pc), a.part_idx = reinterpret_cast<long long *>(b + o_pi);
    long long *d_win = reinterpret_cast<long long *>(b + o_out), *d_ncol = d_win + H;
    double *d_cost = reinterpret_cast<double *>(d_ncol + H);
    const size_t lds = sizeof(double) * 6 * (size_t)plan.CH * (size_t)K;

    c->in_flight = true; c->tail_work = true;
    HIP_TRY(hipMemcpyAsync(b + o_tab, st->up.get(), up_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(st->ev.e0, c->stream));
    for (size_t h0 = 0; h0 < H; h0 += R) {
        a.n_hyp = (int32_t)std::min(R, H - h0);
        a.tables = reinterpret_cast<const double *>(b + o_tab) + h0 * plan.table_words;
        a.winner = d_win + h0, a.n_col = d_ncol + h0, a.cost = d_cost + h0;
        a.out_pred = out->pred ? reinterpret_cast<double *>(b + o_pred) + h0 * n : nullptr;
        a.out_total = out->total ? reinterpret_cast<double *>(b + o_total) + h0 * n : nullptr;
        a.out_col = out->collision ? reinterpret_cast<unsigned char *>(b + o_col) + h0 * n : nullptr;
        HIP_TRY(fx_launch_hypotheses(&a, lds, c->stream));
    }
    HIP_TRY(hipEventRecord(st->ev.e1, c->stream));
    st->ev.timed = true;
    st->CH = plan.CH, st->rounds = plan.rounds, st->launches = plan.launches, st->called = true;
    HIP_TRY(hipMemcpyAsync(st->down.get(), b + o_back, down_bytes, hipMemcpyDeviceToHost, c->stream));   // the one copy back
    FX_TRY(fx_drain(c));
    static_assert(sizeof(long long) == sizeof(int64_t), "the winners are copied as they are");
    const char *d = st->down.get();
    memcpy(out->winner, d + k_ans, sizeof(int64_t) * H);
    if (out->n_collisions) memcpy(out->n_collisions, d + k_ans + sizeof(long long) * H, sizeof(int64_t) * H);
    memcpy(out->cost, d + k_ans + 2 * sizeof(long long) * H, sizeof(double) * H);
    if (out->pred && n > 0) memcpy(out->pred, d + k_pred, sizeof(double) * H * n);
    if (out->total && n > 0) memcpy(out->total, d + k_total, sizeof(double) * H * n);
    if (out->collision && n > 0) memcpy(out->collision, d + k_col, H * n);
    return FX_OK;
}

// device time of the context's last hypotheses call (events around its launches), ms; -1 before the first
double fx_last_hypotheses_ms(FxContext *c) { return (c && c->hyp) ? c->hyp->ev.elapsed_ms() : -1.0; }

int32_t fx_last_hypotheses_info(FxContext *c, int32_t *steps_per_item, int32_t *rounds, int32_t *launches) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!c->hyp || !c->hyp->called) return set_err(FX_ERR_NOT_READY, "no fx_eval_hypotheses_agent call on this context yet");
    if (steps_per_item) *steps_per_item = c->hyp->CH;
    if (rounds) *rounds = c->hyp->rounds;
    if (launches) *launches = c->hyp->launches;
    return FX_OK;
}

}  // extern "C"
