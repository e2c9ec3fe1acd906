// fx_api_rescore.hip -- the last plan step re-scored under many cost-weight vectors at once (header:
// include/fxplan.h; kernels: fx_rescore_kernel.h; launch rule: fx_rescore_plan.h), and the same over EFFECTIVE cost lists and for
// several agents in one call (kernels: fx_rescore_batch_kernel.h; table: fx_rescore_batch_plan.h).  Like the
// sort (fx_api_sort.hip) the pass reads planes of the step -- the raw cost rows and the flag words -- and writes a block of its own.
#include "fx_pass.h"

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

// One agent of a call with its EFFECTIVE cost list: the step's own list with two optional rows from outside the step, pred [C] in
// place of the prediction's row and resp [C] one more term at fx_resp_term_at.  fx_rescore_agent has neither; the table calls
// (fx_rescore_agent_rows, fx_rescore_batch) run rescore_entries below: checks, one staging buffer up, three launches at most,
// winners and costs back in one copy.
struct RescoreEntryCall {
    int32_t agent, n_vec, n_eff, n_pred, at;   // at: position of the responsibility term in the effective list, -1 without one
    const double *w, *pred, *resp;
    int32_t deferred;                          // the sum's form (fx_prediction_term, fx_pass.h): the step deferred its obstacle stage
};

// what every re-score refuses of one agent, in this order, and the effective list; who: "" or "agent 3: "; have_arrays: the arrays
// of the call that may not be NULL are there
static int rescore_entry_check(FxContext *c, const char *who, bool have_arrays, RescoreEntryCall &q) {
    const FxAgentSlot &s = c->slots[q.agent];
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "%splan step ran without FX_MODE_WRITE_COSTMAP", who);
    if (q.n_vec < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "%sn_vec %d", who, q.n_vec);
    if (!have_arrays) return set_err(FX_ERR_INVALID_ARGUMENT, "%sNULL argument", who);
    if (q.n_vec > FX_RESCORE_MAX_VECTORS)
        return set_err(FX_ERR_CAPACITY, "%s%d weight vectors: at most %d per agent", who, q.n_vec, FX_RESCORE_MAX_VECTORS);
    const DevProblem &hp = c->h_probs[q.agent];
    q.n_pred = fx_prediction_term(hp);
    q.deferred = ((hp.mode & FX_MODE_INT_DEFER_OBST) && q.n_pred >= 0) ? 1 : 0;
    if (q.pred && q.n_pred < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "%sa prediction row for a cost list without a prediction term", who);
    q.at = q.resp ? fx_resp_term_at(hp.cost_id, hp.n_cost) : -1;
    q.n_eff = hp.n_cost + (q.resp ? 1 : 0);
    for (size_t k = 0; k < (size_t)q.n_vec * q.n_eff; k++)
        if (!(q.w[k] != 0.0) || !std::isfinite(q.w[k]))
            return set_err(FX_ERR_INVALID_ARGUMENT,
                           "%sweight %d of vector %lld is %g: weights are finite and not zero (a zero weight is another cost list)", who,
                           (int)(k % q.n_eff), (long long)(k / q.n_eff), q.w[k]);
    return FX_OK;
}

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
    FX_TRY(fx_check_inputs_current(c));
    RescoreEntryCall q{agent, n_vec, 0, -1, -1, w, nullptr, nullptr, 0};
    FX_TRY(rescore_entry_check(c, "", w && winner && cost, q));
    FX_TRY(fx_check_not_timed_out(c));
    // (the launch path stays this call's own: the table path costs a descriptor upload more -- DESIGN.md section 24)
    const FxAgentSlot &s = c->slots[agent];
    const int n_cost = q.n_eff;
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
    FX_TRY(fx_pass_room(c, st->block, lay.size()));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block;

    FxRescoreArgs a{};
    a.costmap = c->d_costmap + (size_t)FX_NUM_COSTS * s.cand_off;
    a.flags = c->d_flags + s.cand_off;
    a.n = s.C, a.ld = s.ld, a.n_cost = n_cost, a.n_vec = n_vec;
    a.n_pred = q.n_pred, a.deferred = q.deferred;
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

// the checked entries of a call; winner / cost [sum of n_vec] in call order; totals [n_vec][C] only for a call of one entry
static int rescore_entries(FxContext *c, const std::vector<RescoreEntryCall> &calls, int64_t *winner, double *cost, double *totals) {
    FX_TRY(fx_check_not_timed_out(c));
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
    FX_TRY(fx_pass_room(c, st->block, lay.size(), &st->up, up.size(), &st->down, (sizeof(long long) + sizeof(double)) * V));
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
        e.deferred = q.deferred;
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
    FX_TRY(fx_check_inputs_current(c));
    if (!w || !winner || !cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_agent_rows: NULL argument");
    std::vector<RescoreEntryCall> calls(1, RescoreEntryCall{agent, n_vec, 0, -1, -1, w, pred, resp, 0});
    FX_TRY(rescore_entry_check(c, "", true, calls[0]));
    return rescore_entries(c, calls, winner, cost, totals);
}

int32_t fx_rescore_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const int32_t *n_vec, const double *w,
                         const double *const *pred, const double *const *resp, int64_t *winner, double *cost) {
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_batch: n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;   // (no agent: nothing is touched, the context included)
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!n_vec || !w || !winner || !cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_rescore_batch: NULL argument");
    FX_TRY(check_agent(c, 0));
    FX_TRY(fx_check_inputs_current(c));
    std::vector<RescoreEntryCall> calls((size_t)n_agents);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (int i = 0; i < n_agents; i++) {
        const int32_t agent = agents ? agents[i] : i;
        if (agent < 0 || agent >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
        if (listed[agent]++) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        calls[i] = RescoreEntryCall{agent, n_vec[i], 0, -1, -1, w, pred ? pred[i] : nullptr, resp ? resp[i] : nullptr, 0};
        char who[32];
        snprintf(who, sizeof(who), "agent %d: ", agent);
        FX_TRY(rescore_entry_check(c, who, true, calls[i]));
        w += (size_t)calls[i].n_vec * calls[i].n_eff;
    }
    return rescore_entries(c, calls, winner, cost, nullptr);
}

}  // extern "C"
