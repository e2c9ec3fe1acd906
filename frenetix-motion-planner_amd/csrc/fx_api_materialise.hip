// fx_api_materialise.hip -- listed candidates of the last plan step, materialised beside it (header:
// include/fxplan.h).  fx_materialise_candidates_agent re-walks a caller's list with the step's own arithmetic
// (fx_eval_list_kernel.h) into a compact structure-of-arrays block per agent, the "sparse set"; fx_read_materialised_agent and
// fx_read_package_materialised read it back (the gather kernel of the batched read-back, pointed at the block), the risk passes
// evaluate on it (fx_api_risk.hip).  Nothing here runs in a plan step, and nothing a plan step wrote or published is touched.
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
    std::vector<FxSparseSet> agents;
    FxEventPair ev;   // attached to the last list-kernel launch (fx_last_materialise_ms)
};

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

extern "C" {

int32_t fx_materialise_candidates_agent(FxContext *c, int32_t agent, int64_t n, const int64_t *ids) {
    FX_TRY(check_agent(c, agent));
    const FxAgentSlot &sl = c->slots[agent];
    FX_TRY(fx_check_ids(n, ids, sl.C, "n"));
    if (!fx_inputs_current(c))
        return set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): the re-walk would use another state");
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it");
    if (!c->sparse) c->sparse.reset(new FxSparseState());
    while ((int)c->sparse->agents.size() < c->max_agents) c->sparse->agents.emplace_back(c);
    FxSparseSet &s = c->sparse->agents[agent];
    if (n == 0) { s.ids.clear(); return FX_OK; }

    const DevProblem &src = c->h_probs[agent];
    const int S = sl.S, M = sl.M;
    const size_t lds = fx_generic_lds(M, S, 0);
    if (fx_generic_base_lds(M, S) > 160 * 1024 - 1024)
        return set_err(FX_ERR_CAPACITY, "reference with %d knots does not fit the 160 KiB LDS of the list kernel", M);
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    const int64_t m = (int64_t)sorted.size();
    const int64_t ld = (int64_t)align_up((size_t)m, 64);
    if ((uint64_t)ld * 8u >= (1ull << 32)) return set_err(FX_ERR_CAPACITY, "%lld listed candidates (rows are limited to 4 GiB)", (long long)m);
    const int n_blocks = (int)((m + FX_BLOCK - 1) / FX_BLOCK);
    const size_t n_rows = (size_t)std::max(sl.n_cost, 1);

    // ---- the block: the set's arrays, the kernel's own selection scratch, the list, the clone ----
    FxBlockLayout lay;
    const size_t o_planes = lay.take(sizeof(double) * FX_NUM_PLANES * (size_t)S * ld), o_coeffs = lay.take(sizeof(double) * FX_COEFF_ROWS * ld);
    const size_t o_trajlen = lay.take(sizeof(int32_t) * ld), o_costmap = lay.take(sizeof(double) * n_rows * ld), o_cost = lay.take(sizeof(double) * ld);
    const size_t o_flags = lay.take(sizeof(uint32_t) * ld), o_bstep = lay.take(sizeof(int32_t) * ld);
    const size_t o_cnt = lay.take(sizeof(unsigned long long) * FX_CNT_COUNT), o_pc = lay.take(sizeof(double) * n_blocks);
    const size_t o_pi = lay.take(sizeof(int64_t) * n_blocks), o_ids = lay.take(sizeof(int64_t) * ld), o_prob = lay.take(sizeof(DevProblem));
    HIP_TRY(hipSetDevice(c->device));
    // (the previous call's uploads came from this set's host members: they have landed before those are rewritten)
    FX_TRY(fx_drain(c));
    s.ids.clear();   // from here on the previous set is gone
    FX_TRY(s.block.ensure(lay.size()));
    char *base = s.block;
    s.o_planes = o_planes, s.o_coeffs = o_coeffs, s.o_trajlen = o_trajlen, s.o_costmap = o_costmap, s.o_cost = o_cost;
    s.o_flags = o_flags, s.o_bstep = o_bstep, s.ld = ld;

    DevProblem &d = s.clone;
    d = src;
    d.mode = (src.mode | FX_MODE_WRITE_BUNDLE | FX_MODE_WRITE_COSTMAP) & ~(FX_MODE_INT_DEFER_OBST | FX_MODE_INT_REC_LDS | FX_MODE_INT_STORE_WT);
    d.C = m; d.ld = ld; d.n_blocks = n_blocks;
    d.planes = reinterpret_cast<double *>(base + o_planes);
    d.coeffs = reinterpret_cast<double *>(base + o_coeffs);
    d.traj_len = reinterpret_cast<int32_t *>(base + o_trajlen);
    d.costmap = reinterpret_cast<double *>(base + o_costmap);
    d.cost = reinterpret_cast<double *>(base + o_cost);
    d.flags = reinterpret_cast<uint32_t *>(base + o_flags);
    d.bound_step = reinterpret_cast<int32_t *>(base + o_bstep);
    d.counters = reinterpret_cast<unsigned long long *>(base + o_cnt);
    d.part_cost = reinterpret_cast<double *>(base + o_pc);
    d.part_idx = reinterpret_cast<int64_t *>(base + o_pi);
    d.cost_tail = nullptr; d.obs_part = nullptr; d.obs_colm = nullptr; d.obs_ticket = nullptr; d.obs_list = nullptr;
    d.pkg_out = nullptr; d.pkg_seq = nullptr; d.pkg_plane_rows = 0;
    bool extra = false;
    for (int q = 0; q < d.n_cost; q++) extra |= fx_is_windowed_cost(d.cost_id[q]);
    const bool obst = d.K > 0 || (d.mode & FX_MODE_ROAD_BOUNDARY) != 0;

    int64_t *d_ids = reinterpret_cast<int64_t *>(base + o_ids);
    const DevProblem *d_prob = reinterpret_cast<const DevProblem *>(base + o_prob);
    s.ids.swap(sorted);
    s.step = -1;   // (valid only once everything below was enqueued)
    HIP_TRY(hipMemsetAsync(base + o_cnt, 0, sizeof(unsigned long long) * FX_CNT_COUNT, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ids, s.ids.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(base + o_prob, &d, sizeof(DevProblem), hipMemcpyHostToDevice, c->stream));
    FxSparseState *st = c->sparse.get();
    FX_TRY(st->ev.ensure());
    st->ev.timed = false;
    HIP_TRY(fx_launch_eval_list(d_prob, d_ids, m, lds, obst, extra, st->ev.e0, st->ev.e1, c->stream));
    st->ev.timed = true;
    // the kernel reads the input arena: a state update or an upload behind it waits for the stream first
    c->in_flight = true; c->tail_work = true;
    s.step = c->n_steps;
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
