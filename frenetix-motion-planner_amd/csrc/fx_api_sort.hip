// fx_api_sort.hip -- the stable cost order of all candidates of the last plan step, sorted on the device beside it and read back by
// rank (header: include/fxplan.h; kernels: fx_sort_kernel.h).  Nothing here runs in a plan step, and nothing a
// plan step, the top-k, a sparse set or the risk passes wrote or published is touched: the pass reads the cost and flag planes and
// writes its own block.
#include "fx_pass.h"

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
    FX_TRY(fx_check_inputs_current(c));
    FX_TRY(fx_check_not_timed_out(c));
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
        FX_TRY(fx_pass_room(c, st->block, lay.size()));
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
    FX_TRY(fx_check_not_timed_out(c));
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
