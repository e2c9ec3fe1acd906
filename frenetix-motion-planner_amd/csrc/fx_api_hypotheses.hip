// fx_api_hypotheses.hip -- the obstacle stage of the last plan step run again over many prediction sets at once (DESIGN.md section 25;
// header: include/fxplan.h; kernels: fx_hypotheses_kernel.h; rounds: fx_hypotheses_plan.h), and the same for several agents in one
// call (kernels: fx_hypotheses_batch_kernel.h; rows and rounds: fx_hypotheses_batch_plan.h).  Like the re-score
// (fx_api_rescore.hip) it reads planes of the step -- x, y, theta, the raw cost rows, the flag words -- and writes a block of its own.
#include "fx_pass.h"

static_assert(FX_HYP_MAX == FX_HYPOTHESES_MAX, "fxplan.h states the limit of fx_hypotheses_plan.h");

struct FxHypState {
    explicit FxHypState(FxContext *c) : block(&c->dev_bytes) {}
    FxDeviceBlock block;   // tables of the call (the batch call: and its row tables) | what comes back (answers, then the rows asked
                           // for) | a round's scratch, laid out by FxBlockLayout; both calls share it
    FxEventPair ev;
    FxPinned<char> up, down;   // the tables' staging buffer; everything that comes back, in one copy.  Grow-only
    int32_t CH = 0, rounds = 0, launches = 0;   // of the last call (fx_last_hypotheses_info)
    bool called = false;
};

void fx_hyp_release(FxHypState *s) { delete s; }

// (hook of the tests and of tools/bench_hypotheses.py, not part of fxplan.h: bytes of tables plus scratch per round, 0 = FX_ITEM_SCRATCH_BYTES)
static std::atomic<size_t> fx_hyp_scratch_limit{0};

// what every hypotheses call refuses of one agent, in this order; who: "" or "agent 3: "; fn: the entry's name; have_arrays: the
// arrays of the call that may not be NULL are there
static int hyp_entry_check(FxContext *c, const char *who, const char *fn, int32_t agent, int32_t n_hyp, const FxHypothesis *hyp, bool have_arrays) {
    const FxAgentSlot &s = c->slots[agent];
    const DevProblem &hp = c->h_probs[agent];
    if (!(s.mode & FX_MODE_WRITE_BUNDLE)) return set_err(FX_ERR_NOT_READY, "%splan step ran without FX_MODE_WRITE_BUNDLE", who);
    if (!(s.mode & FX_MODE_WRITE_COSTMAP)) return set_err(FX_ERR_NOT_READY, "%splan step ran without FX_MODE_WRITE_COSTMAP", who);
    if (n_hyp < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "%s%s: n_hyp %d", who, fn, n_hyp);
    if (!have_arrays) return set_err(FX_ERR_INVALID_ARGUMENT, "%s%s: NULL argument", who, fn);
    if (s.K <= 0) return set_err(FX_ERR_INVALID_ARGUMENT, "%sagent %d was uploaded without obstacles (K = 0): upload again", who, agent);
    bool windowed = false;
    for (int m = 0; m < hp.n_cost; m++) windowed |= fx_is_windowed_cost(hp.cost_id[m]);
    // (K <= 64 is also what the tables and the kernels are sized for: one mask word per step, obstacle k on lane k of the cull)
    if (s.K > 64 || (hp.mode & FX_MODE_ROAD_BOUNDARY) || windowed)
        return set_err(FX_ERR_INVALID_ARGUMENT, "%sthe obstacle kernel is not applicable to this step (needs FX_MODE_WRITE_BUNDLE, K <= 64, no road "
                       "boundary, no windowed cost term)", who);
    if (n_hyp > FX_HYP_MAX) return set_err(FX_ERR_CAPACITY, "%s%d hypotheses: at most %d per call", who, n_hyp, FX_HYP_MAX);
    for (int h = 0; h < n_hyp; h++)
        if (!hyp[h].obs_pos || !hyp[h].obs_cov_inv || !hyp[h].obs_npred || !hyp[h].obs_hull || !hyp[h].obs_nhull)
            return set_err(FX_ERR_INVALID_ARGUMENT, "%shypothesis %d: a NULL array (an absent obstacle has obs_npred = 0 and obs_nhull = 0)", who, h);
    return FX_OK;
}

// what the kernels need of the agent's step, the same in both calls: everything of FxHypArgs but a round's own
static FxHypArgs hyp_step_args(const FxAgentSlot &s, const DevProblem &hp, const FxHypPlan &plan) {
    FxHypArgs a{};
    a.planes = hp.planes, a.flags = hp.flags, a.costmap = hp.costmap;
    a.C = s.C, a.ld = s.ld, a.S = hp.S, a.K = s.K;
    a.n_cost = hp.n_cost, a.n_pred = fx_prediction_term(hp);
    for (int m = 0; m < hp.n_cost; m++) a.w[m] = hp.cost_w[m];
    a.deferred = a.n_pred >= 0 ? 1 : 0;   // (without a prediction term the obstacle kernel closes nothing: the walk's own sum)
    a.col_mode = ((hp.mode & FX_MODE_COLLISION) && s.have_hull) ? 1 : 0;
    a.ox = hp.hot_origin[0], a.oy = hp.hot_origin[1];
    a.wb = hp.veh.wb_rear_axle, a.half_len = hp.veh.length / 2, a.half_wid = hp.veh.width / 2;
    a.table_words = plan.table_words, a.CH = plan.CH, a.NC = plan.NC, a.n_tiles = plan.n_tiles, a.n_part = plan.n_part;
    return a;
}

// one table per hypothesis, packed as a state update packs the step's (the step's hot_origin)
static void hyp_pack_table(double *t, const FxAgentSlot &s, const DevProblem &hp, const FxHypothesis &y) {
    const FxHypTable T = fx_hyp_table(hp.S, s.K);
    t[T.margin] = pack_obstacle_tables(hp.S, s.K, s.P, y.obs_pos, y.obs_cov_inv, y.obs_npred, y.obs_hull, y.obs_nhull, s.have_hull,
                                       hp.hot_origin[0], hp.hot_origin[1], t + T.rec, reinterpret_cast<unsigned long long *>(t + T.pm),
                                       reinterpret_cast<unsigned long long *>(t + T.hm), t + T.hot);
}

extern "C" {

void fx_hypotheses_set_scratch_limit(size_t bytes) { fx_hyp_scratch_limit.store(bytes, std::memory_order_relaxed); }

int32_t fx_eval_hypotheses_agent(FxContext *c, int32_t agent, int32_t n_hyp, const FxHypothesis *hyp, const FxHypothesisOutputs *out) {
    // every refusal stands in front of the first allocation, copy or launch
    FX_TRY(check_agent(c, agent));
    FX_TRY(fx_check_inputs_current(c));
    FX_TRY(hyp_entry_check(c, "", "fx_eval_hypotheses_agent", agent, n_hyp, hyp, hyp && out && out->winner && out->cost));
    const FxAgentSlot &s = c->slots[agent];
    const DevProblem &hp = c->h_probs[agent];
    FX_TRY(fx_check_not_timed_out(c));
    const int S = hp.S, K = s.K, CH = c->plan.split_CH;
    const size_t limit_forced = fx_hyp_scratch_limit.load(std::memory_order_relaxed);
    FxHypPlan plan;
    if (!fx_hypotheses_plan(s.C, s.ld, S, K, CH, n_hyp, limit_forced ? limit_forced : FX_ITEM_SCRATCH_BYTES, plan))
        return set_err(FX_ERR_CAPACITY, "%lld candidates: %lld items per hypothesis", (long long)s.C, (long long)plan.items);

    HIP_TRY(hipSetDevice(c->device));
    if (!c->hyp) c->hyp.reset(new FxHypState(c));
    FxHypState *st = c->hyp.get();
    const size_t H = (size_t)n_hyp, R = (size_t)plan.per_round, n = (size_t)s.C, ld = (size_t)s.ld, NC = (size_t)plan.NC;
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
    FX_TRY(fx_pass_room(c, st->block, lay.size(), &st->up, up_bytes, &st->down, down_bytes));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block;

    // one table per hypothesis into one staging buffer
    for (size_t h = 0; h < H; h++) hyp_pack_table(reinterpret_cast<double *>(st->up.get()) + h * plan.table_words, s, hp, hyp[h]);
    FxHypArgs a = hyp_step_args(s, hp, plan);
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

int32_t fx_eval_hypotheses_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const int32_t *n_hyp, const FxHypothesis *hyp,
                                 const FxHypothesisOutputs *out) {
    // every refusal stands in front of the first allocation, copy or launch
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_eval_hypotheses_batch: n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;   // (no agent: nothing is touched, the context included)
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!n_hyp || !hyp || !out || !out->winner || !out->cost) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_eval_hypotheses_batch: NULL argument");
    FX_TRY(check_agent(c, 0));
    FX_TRY(fx_check_inputs_current(c));
    const int E = n_agents;
    std::vector<int32_t> ids((size_t)E);
    std::vector<const FxHypothesis *> first((size_t)E);
    std::vector<FxHypBatchItem> items((size_t)E);
    std::vector<char> listed((size_t)c->n_agents, 0);
    for (int i = 0; i < E; i++) {
        const int32_t agent = agents ? agents[i] : i;
        if (agent < 0 || agent >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
        if (listed[agent]++) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d listed twice", agent);
        char who[32];
        snprintf(who, sizeof(who), "agent %d: ", agent);
        FX_TRY(hyp_entry_check(c, who, "fx_eval_hypotheses_batch", agent, n_hyp[i], hyp, true));
        const FxAgentSlot &s = c->slots[agent];
        ids[i] = agent, first[i] = hyp;
        items[i] = FxHypBatchItem{s.C, s.ld, c->h_probs[agent].S, s.K, n_hyp[i]};
        hyp += n_hyp[i];
    }
    FX_TRY(fx_check_not_timed_out(c));
    const size_t limit_forced = fx_hyp_scratch_limit.load(std::memory_order_relaxed);
    FxHypBatchPlan t;
    int bad = 0;
    if (fx_hypotheses_batch_plan(items.data(), E, c->plan.split_CH, limit_forced ? limit_forced : FX_ITEM_SCRATCH_BYTES, t, &bad))
        // (the hypothesis counts were checked: what is left is a grid)
        return set_err(FX_ERR_CAPACITY, "agent %d: %lld candidates: %lld items per hypothesis", ids[bad], (long long)items[bad].C,
                       (long long)t.plans[bad].items);

    HIP_TRY(hipSetDevice(c->device));
    if (!c->hyp) c->hyp.reset(new FxHypState(c));
    FxHypState *st = c->hyp.get();
    const size_t n_rows = t.rows.size(), P = (size_t)t.pairs;
    // what goes up in ONE copy: all tables of the call | the rows of all rounds | their first workgroups in the three launches
    FxBlockLayout up;
    const size_t u_tab = up.take(t.table_bytes), u_rows = up.take(sizeof(FxHypBatchDevRow) * n_rows), u_first = up.take(sizeof(int64_t) * 3 * n_rows);
    // what comes back in ONE copy, laid out as the caller's arrays are: the agents' answers one behind the other, then their blocks
    // of the rows asked for -- winners [P], counts [P], costs [P] | pred | total | collision
    size_t cells = 0;
    std::vector<size_t> cell0((size_t)E);
    for (int i = 0; i < E; i++) cell0[i] = cells, cells += (size_t)items[i].n_hyp * (size_t)items[i].C;
    FxBlockLayout back;
    const size_t k_ans = back.take(P * (2 * sizeof(long long) + sizeof(double)));
    const size_t k_pred = out->pred ? back.take(sizeof(double) * cells) : 0, k_total = out->total ? back.take(sizeof(double) * cells) : 0;
    const size_t k_col = out->collision ? back.take(cells) : 0;
    FxBlockLayout lay;
    const size_t o_up = lay.take(up.size()), o_back = lay.take(back.size()), o_scr = lay.take(t.scratch);
    FX_TRY(fx_pass_room(c, st->block, lay.size(), &st->up, up.size(), &st->down, back.size()));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    char *b = st->block, *h = st->up.get();
    long long *d_win = reinterpret_cast<long long *>(b + o_back + k_ans), *d_ncol = d_win + P;
    double *d_cost = reinterpret_cast<double *>(d_ncol + P);

    for (int i = 0; i < E; i++) {
        const FxAgentSlot &s = c->slots[ids[i]];
        for (int32_t y = 0; y < items[i].n_hyp; y++)
            hyp_pack_table(reinterpret_cast<double *>(h + u_tab + t.table0[i]) + (size_t)y * t.plans[i].table_words, s, c->h_probs[ids[i]], first[i][y]);
    }
    FxHypBatchDevRow *rows = reinterpret_cast<FxHypBatchDevRow *>(h + u_rows);
    int64_t *first0 = reinterpret_cast<int64_t *>(h + u_first);
    for (size_t k = 0; k < n_rows; k++) {
        const FxHypBatchRow &r = t.rows[k];
        const int i = r.entry;
        const FxAgentSlot &s = c->slots[ids[i]];
        const FxHypPlan &plan = t.plans[i];
        const FxHypSegment g = fx_hyp_batch_segment(plan, s.ld, r.n_hyp);
        char *seg = b + o_scr + r.scratch_off;
        const size_t cell = cell0[i] + (size_t)r.h0 * (size_t)s.C;
        FxHypBatchDevRow d{};
        d.a = hyp_step_args(s, c->h_probs[ids[i]], plan);
        d.a.tables = reinterpret_cast<const double *>(b + o_up + u_tab + r.table_off);
        d.a.n_hyp = r.n_hyp;
        d.a.part = reinterpret_cast<double *>(seg + g.part), d.a.colm = reinterpret_cast<unsigned long long *>(seg + g.colm);
        d.a.tot = reinterpret_cast<double *>(seg + g.tot), d.a.colb = reinterpret_cast<unsigned char *>(seg + g.colb);
        d.a.part_cost = reinterpret_cast<double *>(seg + g.part_cost), d.a.part_idx = reinterpret_cast<long long *>(seg + g.part_idx);
        d.a.winner = d_win + r.out0, d.a.n_col = d_ncol + r.out0, d.a.cost = d_cost + r.out0;
        d.a.out_pred = out->pred ? reinterpret_cast<double *>(b + o_back + k_pred) + cell : nullptr;
        d.a.out_total = out->total ? reinterpret_cast<double *>(b + o_back + k_total) + cell : nullptr;
        d.a.out_col = out->collision ? reinterpret_cast<unsigned char *>(b + o_back + k_col) + cell : nullptr;
        d.item0 = r.item0, d.fin0 = r.fin0, d.sel0 = r.sel0, d.items = plan.items;
        rows[k] = d;
        first0[k] = r.item0, first0[n_rows + k] = r.fin0, first0[2 * n_rows + k] = r.sel0;
    }

    c->in_flight = true; c->tail_work = true;
    HIP_TRY(hipMemcpyAsync(b + o_up, h, up.size(), hipMemcpyHostToDevice, c->stream));   // the one copy up
    HIP_TRY(hipEventRecord(st->ev.e0, c->stream));
    const int64_t *d_first = reinterpret_cast<const int64_t *>(b + o_up + u_first);
    for (const FxHypBatchRound &rd : t.rounds) {
        FxHypBatchArgs a{};
        a.rows = reinterpret_cast<const FxHypBatchDevRow *>(b + o_up + u_rows) + rd.row0;
        a.item0 = d_first + rd.row0, a.fin0 = d_first + n_rows + rd.row0, a.sel0 = d_first + 2 * n_rows + rd.row0;
        a.n_rows = rd.n_rows, a.CH = t.CH;
        a.items = rd.items, a.fin_blocks = rd.fin_blocks, a.pairs = rd.pairs;
        a.lds_bytes = sizeof(double) * 6 * (size_t)t.CH * (size_t)rd.K_max;
        HIP_TRY(fx_launch_hypotheses_batch(&a, c->stream));
    }
    HIP_TRY(hipEventRecord(st->ev.e1, c->stream));
    st->ev.timed = true;
    st->CH = t.CH, st->rounds = (int32_t)t.rounds.size(), st->launches = t.launches, st->called = true;
    HIP_TRY(hipMemcpyAsync(st->down.get(), b + o_back, back.size(), hipMemcpyDeviceToHost, c->stream));   // the one copy back
    FX_TRY(fx_drain(c));
    const char *d = st->down.get();
    memcpy(out->winner, d + k_ans, sizeof(int64_t) * P);
    if (out->n_collisions) memcpy(out->n_collisions, d + k_ans + sizeof(long long) * P, sizeof(int64_t) * P);
    memcpy(out->cost, d + k_ans + 2 * sizeof(long long) * P, sizeof(double) * P);
    if (out->pred && cells > 0) memcpy(out->pred, d + k_pred, sizeof(double) * cells);
    if (out->total && cells > 0) memcpy(out->total, d + k_total, sizeof(double) * cells);
    if (out->collision && cells > 0) memcpy(out->collision, d + k_col, cells);
    return FX_OK;
}

// device time of the context's last hypotheses call of either kind (events around its launches), ms; -1 before the first
double fx_last_hypotheses_ms(FxContext *c) { return (c && c->hyp) ? c->hyp->ev.elapsed_ms() : -1.0; }

int32_t fx_last_hypotheses_info(FxContext *c, int32_t *steps_per_item, int32_t *rounds, int32_t *launches) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!c->hyp || !c->hyp->called) return set_err(FX_ERR_NOT_READY, "no fx_eval_hypotheses_agent or fx_eval_hypotheses_batch call on this context yet");
    if (steps_per_item) *steps_per_item = c->hyp->CH;
    if (rounds) *rounds = c->hyp->rounds;
    if (launches) *launches = c->hyp->launches;
    return FX_OK;
}

}  // extern "C"
