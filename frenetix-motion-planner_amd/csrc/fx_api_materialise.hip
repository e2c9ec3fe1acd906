// fx_api_materialise.hip -- listed candidates of the last plan step, materialised beside it (header:
// include/fxplan.h).  fx_materialise_candidates_agent re-walks a caller's list with the step's own arithmetic
// (fx_eval_list_kernel.h) into a compact structure-of-arrays block per agent, the "sparse set"; fx_read_materialised_agent and
// fx_read_package_materialised read it back (the gather kernel of the batched read-back, pointed at the block), the risk passes
// evaluate on it (fx_api_risk.hip).  fx_materialise_candidates_batch makes the sets of several agents in one call and
// fx_set_materialise_lanes splits a candidate's horizon over 8 or 32 lanes (the rows form of the list kernel).
// Nothing here runs in a plan step, and nothing a plan step wrote or published is touched.
#include "fx_pass.h"

// One agent's set.  `ids` is kept ascending and de-duplicated: positions are monotone in the candidate index, so an arg-min over
// positions with ties to the lower position is the arg-min over candidates with ties to the lower index.
struct FxSparseSet {
    explicit FxSparseSet(FxContext *c) : block(&c->dev_bytes) {}
    std::vector<int64_t> ids;
    long long step = -1;      // FxContext.n_steps when the set was made: the next evaluation ends it
    FxDeviceBlock block;      // every part 256-byte aligned (FxBlockLayout)
    int64_t ld = 0;
    size_t o_planes = 0, o_coeffs = 0, o_trajlen = 0, o_costmap = 0, o_cost = 0, o_flags = 0, o_bstep = 0;
    DevProblem clone;         // host copy of the problem the list kernel was launched with
};

struct FxSparseState {
    explicit FxSparseState(FxContext *c) : call(&c->dev_bytes) {}
    std::vector<FxSparseSet> agents;
    FxEventPair ev;   // around the last call's launch sequence (fx_last_materialise_ms)
    int lanes = 1;    // fx_set_materialise_lanes: 1, 8 or 32 lanes per candidate
    int last_lanes = 0, last_launches = 0, last_rows = 0;   // fx_last_materialise_info
    // the rows form (section 22): row table, clones, lists and the kernel's selection scratch of ONE call, built in the pinned
    // block and sent in one copy; both grow-only
    FxDeviceBlock call;
    FxPinned<char> h_call;
};

static FxSparseState *sparse_state(FxContext *c) {
    if (!c->sparse) c->sparse.reset(new FxSparseState(c));
    while ((int)c->sparse->agents.size() < c->max_agents) c->sparse->agents.emplace_back(c);
    return c->sparse.get();
}

// the parts of a set that its consumers read (FxSparseView), in the order and alignment of the per-agent call's block
struct FxSparseOutputs {
    size_t o_planes, o_coeffs, o_trajlen, o_costmap, o_cost, o_flags, o_bstep;
    void take(FxBlockLayout &lay, int S, size_t n_rows, int64_t ld) {
        o_planes = lay.take(sizeof(double) * FX_NUM_PLANES * (size_t)S * ld), o_coeffs = lay.take(sizeof(double) * FX_COEFF_ROWS * ld);
        o_trajlen = lay.take(sizeof(int32_t) * ld), o_costmap = lay.take(sizeof(double) * n_rows * ld), o_cost = lay.take(sizeof(double) * ld);
        o_flags = lay.take(sizeof(uint32_t) * ld), o_bstep = lay.take(sizeof(int32_t) * ld);
    }
};

// the clone of an agent's problem the list kernels run on: m listed candidates in columns of `base` at `o`, n_blocks workgroups
static void fx_sparse_clone(DevProblem &d, const DevProblem &src, int64_t m, int64_t ld, int n_blocks, char *base, const FxSparseOutputs &o,
                            unsigned long long *counters, double *part_cost, int64_t *part_idx) {
    d = src;
    d.mode = (src.mode | FX_MODE_WRITE_BUNDLE | FX_MODE_WRITE_COSTMAP) & ~(FX_MODE_INT_DEFER_OBST | FX_MODE_INT_REC_LDS | FX_MODE_INT_STORE_WT | FX_MODE_INT_CHUNK_INDEX);
    d.C = m; d.ld = ld; d.n_blocks = n_blocks;
    d.planes = reinterpret_cast<double *>(base + o.o_planes);
    d.coeffs = reinterpret_cast<double *>(base + o.o_coeffs);
    d.traj_len = reinterpret_cast<int32_t *>(base + o.o_trajlen);
    d.costmap = reinterpret_cast<double *>(base + o.o_costmap);
    d.cost = reinterpret_cast<double *>(base + o.o_cost);
    d.flags = reinterpret_cast<uint32_t *>(base + o.o_flags);
    d.bound_step = reinterpret_cast<int32_t *>(base + o.o_bstep);
    d.counters = counters;
    d.part_cost = part_cost;
    d.part_idx = part_idx;
    d.cost_tail = nullptr; d.obs_part = nullptr; d.obs_colm = nullptr; d.obs_ticket = nullptr; d.obs_list = nullptr;
    d.pkg_out = nullptr; d.pkg_seq = nullptr; d.pkg_plane_rows = 0;
}

static bool fx_sparse_windowed(const DevProblem &d) {
    bool extra = false;
    for (int q = 0; q < d.n_cost; q++) extra |= fx_is_windowed_cost(d.cost_id[q]);
    return extra;
}

void fx_sparse_release(FxSparseState *s) { delete s; }

bool fx_sparse_view(FxContext *c, int32_t agent, FxSparseView *v) {
    if (!c || !c->sparse || agent < 0 || agent >= (int)c->sparse->agents.size()) return false;
    const FxSparseSet &s = c->sparse->agents[agent];
    if (s.ids.empty() || s.step != c->n_steps || !fx_inputs_current(c)) return false;
    v->ids = s.ids.data();
    v->n = (int64_t)s.ids.size();
    v->ld = s.ld;
    v->planes = reinterpret_cast<const double *>(s.block + s.o_planes);
    v->coeffs = reinterpret_cast<const double *>(s.block + s.o_coeffs);
    v->costmap = reinterpret_cast<const double *>(s.block + s.o_costmap);
    v->cost = reinterpret_cast<const double *>(s.block + s.o_cost);
    v->flags = reinterpret_cast<const uint32_t *>(s.block + s.o_flags);
    v->traj_len = reinterpret_cast<const int32_t *>(s.block + s.o_trajlen);
    v->bound_step = reinterpret_cast<const int32_t *>(s.block + s.o_bstep);
    return true;
}

bool fx_sparse_positions(const FxSparseView &v, int64_t n, const int64_t *ids, std::vector<int64_t> &pos) {
    pos.resize((size_t)std::max<int64_t>(n, 0));
    for (int64_t j = 0; j < n; j++) {
        const int64_t *at = std::lower_bound(v.ids, v.ids + v.n, ids[j]);
        if (at == v.ids + v.n || *at != ids[j]) return false;
        pos[(size_t)j] = (int64_t)(at - v.ids);
    }
    return true;
}

// What both calls check of one listed agent behind its list (fx_check_ids: the caller's) and before anything is written, and what
// they need of it afterwards
struct FxSparsePlan {
    int32_t agent;
    std::vector<int64_t> sorted;   // ascending, de-duplicated
    int64_t m, ld;
    int lanes, n_blocks;           // lanes per candidate of this agent's kernel; its workgroups
    bool obst, extra;
    size_t lds;
};
static int fx_sparse_plan(FxContext *c, int32_t agent, int64_t n, const int64_t *ids, int lanes_set, FxSparsePlan &p) {
    const FxAgentSlot &sl = c->slots[agent];
    p.agent = agent;
    p.m = 0;
    if (n == 0) return FX_OK;
    const DevProblem &src = c->h_probs[agent];
    if (fx_generic_base_lds(sl.M, sl.S) > 160 * 1024 - 1024)
        return set_err(FX_ERR_CAPACITY, "reference with %d knots does not fit the 160 KiB LDS of the list kernel", sl.M);
    p.lds = fx_generic_lds(sl.M, sl.S, 0);
    p.sorted.assign(ids, ids + n);
    std::sort(p.sorted.begin(), p.sorted.end());
    p.sorted.erase(std::unique(p.sorted.begin(), p.sorted.end()), p.sorted.end());
    p.m = (int64_t)p.sorted.size();
    p.ld = (int64_t)align_up((size_t)p.m, 64);
    if ((uint64_t)p.ld * 8u >= (1ull << 32)) return set_err(FX_ERR_CAPACITY, "%lld listed candidates (rows are limited to 4 GiB)", (long long)p.m);
    p.extra = fx_sparse_windowed(src);
    p.obst = src.K > 0 || (src.mode & FX_MODE_ROAD_BOUNDARY) != 0;
    p.lanes = p.extra ? 1 : lanes_set;   // (windowed terms need the whole horizon in one lane)
    const int cpb = FX_BLOCK / p.lanes;
    p.n_blocks = (int)((p.m + cpb - 1) / cpb);
    return FX_OK;
}
static int fx_sparse_ready(FxContext *c) {
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): the re-walk would use another state");
    return fx_check_not_timed_out(c);
}

// The rows form: every plan with candidates becomes a row of its variant's launch.  Everything was checked; from here on only the
// runtime can fail.  One drain, one upload, one launch per variant present.
static int fx_sparse_run_rows(FxContext *c, std::vector<FxSparsePlan> &plans) {
    FxSparseState *st = sparse_state(c);
    // rows in launch order: by variant (lanes, obst, extra), agents of one variant in call order
    std::vector<int> order;
    for (int j = 0; j < (int)plans.size(); j++)
        if (plans[j].m > 0) order.push_back(j);
    auto variant = [&](int j) { return std::make_tuple(plans[j].lanes, plans[j].obst, plans[j].extra); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return variant(a) < variant(b); });
    const size_t R = order.size();

    // ---- the call's block: the row table, then per row the kernel's selection scratch, the list and the clone ----
    struct RowAt { size_t o_cnt, o_pc, o_pi, o_ids, o_prob; };
    std::vector<RowAt> at(R);
    FxBlockLayout lay;
    const size_t o_rows = lay.take(sizeof(EvalListRow) * R);
    for (size_t r = 0; r < R; r++) {
        const FxSparsePlan &p = plans[order[r]];
        at[r].o_cnt = lay.take(sizeof(unsigned long long) * FX_CNT_COUNT), at[r].o_pc = lay.take(sizeof(double) * p.n_blocks);
        at[r].o_pi = lay.take(sizeof(int64_t) * p.n_blocks), at[r].o_ids = lay.take(sizeof(int64_t) * p.ld), at[r].o_prob = lay.take(sizeof(DevProblem));
    }
    HIP_TRY(hipSetDevice(c->device));
    // (the previous call's upload came from the pinned block and the sets' host members: it has landed before those are rewritten)
    FX_TRY(fx_drain(c));
    for (FxSparsePlan &p : plans) st->agents[p.agent].ids.clear();   // from here on the previous sets of the listed agents are gone
    st->last_lanes = st->last_launches = st->last_rows = 0;
    st->ev.timed = false;
    if (R == 0) return FX_OK;
    FX_TRY(st->call.ensure(lay.size()));
    FX_TRY(st->h_call.ensure(lay.size(), hipHostMallocDefault));
    char *h = st->h_call, *d = st->call;
    EvalListRow *h_rows = reinterpret_cast<EvalListRow *>(h + o_rows);
    for (size_t r = 0; r < R; r++) {
        FxSparsePlan &p = plans[order[r]];
        const FxAgentSlot &sl = c->slots[p.agent];
        FxSparseSet &s = st->agents[p.agent];
        FxBlockLayout own;
        FxSparseOutputs o;
        o.take(own, sl.S, (size_t)std::max(sl.n_cost, 1), p.ld);
        FX_TRY(s.block.ensure(own.size()));
        s.o_planes = o.o_planes, s.o_coeffs = o.o_coeffs, s.o_trajlen = o.o_trajlen, s.o_costmap = o.o_costmap, s.o_cost = o.o_cost;
        s.o_flags = o.o_flags, s.o_bstep = o.o_bstep, s.ld = p.ld;
        fx_sparse_clone(s.clone, c->h_probs[p.agent], p.m, p.ld, p.n_blocks, s.block, o, reinterpret_cast<unsigned long long *>(d + at[r].o_cnt),
                        reinterpret_cast<double *>(d + at[r].o_pc), reinterpret_cast<int64_t *>(d + at[r].o_pi));
        memset(h + at[r].o_cnt, 0, sizeof(unsigned long long) * FX_CNT_COUNT);
        memcpy(h + at[r].o_ids, p.sorted.data(), sizeof(int64_t) * p.m);
        memcpy(h + at[r].o_prob, &s.clone, sizeof(DevProblem));
        h_rows[r] = EvalListRow{reinterpret_cast<const DevProblem *>(d + at[r].o_prob), reinterpret_cast<const int64_t *>(d + at[r].o_ids)};
        s.ids.swap(p.sorted);
        s.step = -1;   // (valid only once everything below was enqueued)
    }
    HIP_TRY(hipMemcpyAsync(d, h, lay.size(), hipMemcpyHostToDevice, c->stream));
    FX_TRY(st->ev.ensure());
    int launches = 0, lanes = 0;
    for (size_t r0 = 0; r0 < R;) {
        size_t r1 = r0;
        int64_t n_max = 0;
        size_t lds = 0;
        while (r1 < R && variant(order[r1]) == variant(order[r0])) {
            n_max = std::max(n_max, plans[order[r1]].m), lds = std::max(lds, plans[order[r1]].lds);
            r1++;
        }
        const FxSparsePlan &p = plans[order[r0]];
        HIP_TRY(fx_launch_eval_list(nullptr, nullptr, n_max, lds, p.obst, p.extra, reinterpret_cast<const EvalListRow *>(d + o_rows) + r0,
                                    (int)(r1 - r0), p.lanes, r0 == 0 ? (hipEvent_t)st->ev.e0 : nullptr, r1 == R ? (hipEvent_t)st->ev.e1 : nullptr,
                                    c->stream));
        launches++;
        lanes = std::max(lanes, p.lanes);
        r0 = r1;
    }
    st->ev.timed = true;
    st->last_lanes = lanes, st->last_launches = launches, st->last_rows = (int)R;
    // the kernels read the input arena: a state update or an upload behind them waits for the stream first
    c->in_flight = true; c->tail_work = true;
    for (size_t r = 0; r < R; r++) st->agents[plans[order[r]].agent].step = c->n_steps;
    return FX_OK;
}

extern "C" {

int32_t fx_materialise_candidates_agent(FxContext *c, int32_t agent, int64_t n, const int64_t *ids) {
    FX_TRY(check_agent(c, agent));
    const FxAgentSlot &sl = c->slots[agent];
    const int lanes_set = c->sparse ? c->sparse->lanes : 1;
    FX_TRY(fx_check_ids(n, ids, sl.C, "n"));
    FX_TRY(fx_sparse_ready(c));
    FxSparseState *st = sparse_state(c);
    FxSparseSet &s = st->agents[agent];
    if (n == 0) { s.ids.clear(); return FX_OK; }
    std::vector<FxSparsePlan> plans(1);
    FxSparsePlan &p = plans[0];
    FX_TRY(fx_sparse_plan(c, agent, n, ids, lanes_set, p));
    if (p.lanes > 1) return fx_sparse_run_rows(c, plans);   // split lanes: the rows form with one row

    const int S = sl.S;
    const int64_t m = p.m, ld = p.ld;
    const int n_blocks = p.n_blocks;

    // ---- the block: the set's arrays, the kernel's own selection scratch, the list, the clone ----
    FxBlockLayout lay;
    FxSparseOutputs o;
    o.take(lay, S, (size_t)std::max(sl.n_cost, 1), ld);
    const size_t o_cnt = lay.take(sizeof(unsigned long long) * FX_CNT_COUNT), o_pc = lay.take(sizeof(double) * n_blocks);
    const size_t o_pi = lay.take(sizeof(int64_t) * n_blocks), o_ids = lay.take(sizeof(int64_t) * ld), o_prob = lay.take(sizeof(DevProblem));
    HIP_TRY(hipSetDevice(c->device));
    // (the previous call's uploads came from this set's host members: they have landed before those are rewritten)
    FX_TRY(fx_drain(c));
    s.ids.clear();   // from here on the previous set is gone
    FX_TRY(s.block.ensure(lay.size()));
    char *base = s.block;
    s.o_planes = o.o_planes, s.o_coeffs = o.o_coeffs, s.o_trajlen = o.o_trajlen, s.o_costmap = o.o_costmap, s.o_cost = o.o_cost;
    s.o_flags = o.o_flags, s.o_bstep = o.o_bstep, s.ld = ld;

    DevProblem &d = s.clone;
    fx_sparse_clone(d, c->h_probs[agent], m, ld, n_blocks, base, o, reinterpret_cast<unsigned long long *>(base + o_cnt),
                    reinterpret_cast<double *>(base + o_pc), reinterpret_cast<int64_t *>(base + o_pi));

    int64_t *d_ids = reinterpret_cast<int64_t *>(base + o_ids);
    const DevProblem *d_prob = reinterpret_cast<const DevProblem *>(base + o_prob);
    s.ids.swap(p.sorted);
    s.step = -1;   // (valid only once everything below was enqueued)
    HIP_TRY(hipMemsetAsync(base + o_cnt, 0, sizeof(unsigned long long) * FX_CNT_COUNT, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ids, s.ids.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(base + o_prob, &d, sizeof(DevProblem), hipMemcpyHostToDevice, c->stream));
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    st->last_lanes = st->last_launches = st->last_rows = 0;
    HIP_TRY(fx_launch_eval_list(d_prob, d_ids, m, p.lds, p.obst, p.extra, nullptr, 0, 1, st->ev.e0, st->ev.e1, c->stream));
    st->ev.timed = true;
    st->last_lanes = st->last_launches = st->last_rows = 1;
    // the kernel reads the input arena: a state update or an upload behind it waits for the stream first
    c->in_flight = true; c->tail_work = true;
    s.step = c->n_steps;
    return FX_OK;
}

int32_t fx_set_materialise_lanes(FxContext *c, int32_t lanes) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (lanes != 0 && lanes != 1 && lanes != 8 && lanes != 32)
        return set_err(FX_ERR_INVALID_ARGUMENT, "materialise lanes %d: one of 0, 1, 8, 32", lanes);
    sparse_state(c)->lanes = lanes == 0 ? 1 : lanes;
    return FX_OK;
}

int32_t fx_materialise_candidates_batch(FxContext *c, int32_t n_agents, const int32_t *agents, const int64_t *n_ids, const int64_t *const *ids) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (n_agents < 0) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d", n_agents);
    if (n_agents == 0) return FX_OK;
    if (!n_ids || !ids) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_materialise_candidates_batch: NULL n_ids or ids");
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "no evaluated plan step");
    if (n_agents > c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "n_agents %d, the last upload holds %d", n_agents, c->n_agents);
    const int lanes_set = c->sparse ? c->sparse->lanes : 1;
    std::vector<FxSparsePlan> plans((size_t)n_agents);
    std::vector<char> seen((size_t)c->n_agents, 0);
    for (int j = 0; j < n_agents; j++) {
        const int32_t a = agents ? agents[j] : j;
        if (a < 0 || a >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", a);
        if (seen[a]++) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d is listed twice", a);
        FX_TRY(fx_check_ids(n_ids[j], ids[j], c->slots[a].C, "n_ids"));
    }
    FX_TRY(fx_sparse_ready(c));
    for (int j = 0; j < n_agents; j++)
        FX_TRY(fx_sparse_plan(c, agents ? agents[j] : j, n_ids[j], ids[j], lanes_set, plans[(size_t)j]));
    return fx_sparse_run_rows(c, plans);
}

int32_t fx_last_materialise_info(FxContext *c, int32_t *lanes, int32_t *launches, int32_t *rows) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    const FxSparseState *st = c->sparse.get();
    if (lanes) *lanes = st ? st->last_lanes : 0;
    if (launches) *launches = st ? st->last_launches : 0;
    if (rows) *rows = st ? st->last_rows : 0;
    return FX_OK;
}

int32_t fx_read_materialised_agent(FxContext *c, int32_t agent, int64_t n, const int64_t *ids, double *planes, double *coeffs13,
                                   int32_t *traj_len, double *raw_costs, double *cost, uint32_t *flags, int32_t *boundary_step) {
    FX_TRY(check_agent(c, agent));
    const FxAgentSlot &sl = c->slots[agent];
    FX_TRY(fx_check_ids(n, ids, sl.C, "n"));
    if (boundary_step && !(sl.mode & FX_MODE_ROAD_BOUNDARY)) return set_err(FX_ERR_NOT_READY, "the step ran without FX_MODE_ROAD_BOUNDARY");
    if (n == 0) return FX_OK;
    FxSparseView v;
    std::vector<int64_t> pos;
    if (!fx_sparse_view(c, agent, &v) || !fx_sparse_positions(v, n, ids, pos))
        return set_err(FX_ERR_NOT_READY, "a listed candidate is not in the agent's materialised set (fx_materialise_candidates_agent)");
    GatherArgs ga;
    ga.planes = v.planes; ga.coeffs = v.coeffs; ga.costmap = v.costmap; ga.cost = v.cost; ga.flags = v.flags; ga.traj_len = v.traj_len;
    ga.bound_step = v.bound_step;
    ga.ld = v.ld; ga.C = v.n; ga.S = sl.S; ga.n_cost = sl.n_cost;
    ga.parts = ((planes || coeffs13 || traj_len) ? FX_GATHER_BUNDLE : 0u) | ((raw_costs && sl.n_cost > 0) ? FX_GATHER_COSTMAP : 0u) |
               (boundary_step ? FX_GATHER_BOUNDARY : 0u);
    return fx_gather_rows(c, ga, n, pos.data(), planes, coeffs13, traj_len, raw_costs, cost, flags, boundary_step);
}

int32_t fx_read_package_materialised(FxContext *c, int32_t agent, int64_t index, double yaw_rate0, FxPackage *pkg, double *block) {
    FX_TRY(check_agent(c, agent));
    if (!pkg) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_read_package_materialised: NULL argument");
    const FxAgentSlot &sl = c->slots[agent];
    const DevProblem &d = c->h_probs[agent];
    double co[FX_COEFF_ROWS], raw[FX_NUM_COSTS] = {0.0}, cost = 0.0;
    int32_t tl = 0;
    uint32_t fl = 0;
    std::vector<double> own;   // (planes are read either way: one record, one copy)
    if (!block) { own.resize((size_t)FX_NUM_PLANES * sl.S); }
    FX_TRY(fx_read_materialised_agent(c, agent, 1, &index, block ? block : own.data(), co, &tl, raw, &cost, &fl, nullptr));
    memset(pkg, 0, sizeof(*pkg));
    pkg->found = 1;
    pkg->S = sl.S;
    pkg->n_cost = sl.n_cost;
    pkg->index = index + d.g_base;
    memcpy(pkg->coeff_lon, co, sizeof(double) * 6);
    memcpy(pkg->coeff_lat, co + 6, sizeof(double) * 6);
    memcpy(pkg->raw_costs, raw, sizeof(double) * FX_NUM_COSTS);
    pkg->cost = cost;
    pkg->traj_len = tl;
    pkg->flags = fl;
    pkg->tau_lat = co[12];
    if (block) fx_package_derive(d, sl.S, yaw_rate0, block);
    return FX_OK;
}

// device time of the last list-kernel launch of this context (events attached to the kernel itself), ms; -1 before the first
double fx_last_materialise_ms(FxContext *c) { return (c && c->sparse) ? c->sparse->ev.elapsed_ms() : -1.0; }

}  // extern "C"
