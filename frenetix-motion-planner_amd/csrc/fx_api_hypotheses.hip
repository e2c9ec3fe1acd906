// fx_api_hypotheses.hip -- the obstacle stage of the last plan step run again over many prediction sets at once (DESIGN.md section 25;
// header: include/fxplan.h; kernels: fx_hypotheses_kernel.h; rounds: fx_hypotheses_plan.h).  Like the re-score (fx_api_rescore.hip) it
// reads planes of the step -- x, y, theta, the raw cost rows, the flag words -- and writes a block of its own.
#include "fx_pass.h"

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
    FX_TRY(fx_check_inputs_current(c));
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
    FX_TRY(fx_check_not_timed_out(c));
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
    FX_TRY(fx_pass_room(c, st->block, lay.size(), &st->up, up_bytes, &st->down, down_bytes));
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
    a.n_cost = hp.n_cost, a.n_pred = fx_prediction_term(hp);
    for (int m = 0; m < hp.n_cost; m++) a.w[m] = hp.cost_w[m];
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
