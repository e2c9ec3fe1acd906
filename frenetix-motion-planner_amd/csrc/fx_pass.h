// fx_pass.h -- the host scaffold of the passes that run beside the plan step (fx_api_risk.hip, fx_api_sort.hip, fx_api_rescore.hip,
// fx_api_hypotheses.hip, fx_api_materialise.hip, the read-back of fx_api_host.hip), each piece written once.  Nothing here launches a kernel.  The block of
// a pass is an FxDeviceBlock (fx_owner.h): grow-only, laid out by FxBlockLayout.
#pragma once

#include "fx_context.h"

#define FX_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// The parts of one device block, every part 256-byte aligned and at least 8 bytes.  Pure: no HIP call (tests/policy_table.cpp).
struct FxBlockLayout {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align_up(std::max<size_t>(bytes, 8), 256); return o; }
    size_t size() const { return off; }
};

// The events around a pass's launches, created on first use.  `timed`: they bracket a launch sequence that was enqueued whole.
struct FxEventPair {
    FxEvent e0, e1;
    bool timed = false;
    int ensure() {
        FX_TRY(e0.create());
        return e1.create();
    }
    // device time between the two, ms (waits for the second one); -1 before the first timed launch and on any failure
    double elapsed_ms() const {
        float ms = -1.f;
        if (timed && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) { (void)hipGetLastError(); ms = -1.f; }
        return (double)ms;
    }
};

// Steps per chunk of an item decomposition -- one wave per (tile of 64 candidates, chunk of steps, obstacle) -- over n candidates,
// S - 1 steps and K obstacles: as many as keep the call at FX_ITEM_WAVES items or more, at least one -- or `forced` > 0, a test's
// choice.  The one rule of the prediction-probability items and the risk items (both fx_api_risk.hip).  Pure: no HIP call.
#define FX_ITEM_WAVES 4096
inline int fx_item_chunk_steps(int64_t n, int S, int K, int forced) {
    const int steps = S - 1 > 0 ? S - 1 : 1;
    if (forced > 0) return std::min(forced, steps);
    const int64_t per_step = ((n + 63) / 64) * std::max(K, 1);   // items of a call with one step per chunk
    int cs = 1;
    while (cs < steps && per_step * ((steps + 2 * cs - 1) / (2 * cs)) >= FX_ITEM_WAVES) cs *= 2;
    return std::min(cs, steps);
}

// Candidates per batch of such a pass, whose scratch -- the per-step probabilities of fx_eval_prediction_prob_agent, the partials
// of the risk items -- holds one batch at per_candidate_bytes each: whole tiles of 64; at most FX_ITEM_SCRATCH_BYTES of scratch
// where one candidate's share allows; never more tiles than the call's n candidates have.  Pure: no HIP call.
#define FX_ITEM_SCRATCH_BYTES ((size_t)64 << 20)
inline int64_t fx_item_batch(size_t per_candidate_bytes, int64_t n) {
    const size_t tiles = std::max<size_t>(FX_ITEM_SCRATCH_BYTES / per_candidate_bytes / 64, 1);
    const size_t call = ((size_t)std::max<int64_t>(n, 1) + 63) / 64;
    return (int64_t)(std::min(tiles, call) * 64);
}

// The rounds of such a pass over SEVERAL agents in one call (the four batched entries of fx_api_risk.hip): the scratch of one round holds
// segments of candidates of one or more agents, at most `limit` bytes of it.  agents: per agent its n candidates and one
// candidate's share of the scratch in bytes (0: the agent needs none).  The rule:
//   * agents in call order, each agent's candidates ascending and contiguous;
//   * a segment's scratch is whole tiles of 64 candidates, and every segment but an agent's last is whole tiles;
//   * a round is closed only when the next tile does not fit; a tile that alone exceeds the limit is a round by itself
//     (fx_item_batch's "at least one tile").
// An agent has at most one segment per round; an agent without candidates has none.  Pure: no HIP call (tests/item_rounds.cpp).
struct FxItemAgent {
    int64_t n;
    size_t per_candidate_bytes;
};
struct FxItemSegment {
    int32_t agent, round;   // position in the call's list; rounds count from 0
    int64_t first, count;   // candidates [first, first + count) of the agent
    size_t scratch_off;     // bytes, from the start of the round's scratch
};
inline std::vector<FxItemSegment> fx_item_rounds(const FxItemAgent *agents, int n_agents, size_t limit) {
    std::vector<FxItemSegment> segs;
    int32_t round = 0;
    size_t used = 0;
    for (int a = 0; a < n_agents; a++) {
        const size_t tile = 64 * agents[a].per_candidate_bytes;
        for (int64_t j = 0; j < agents[a].n; j += 64) {
            if (used > 0 && tile > limit - std::min(used, limit)) { round++; used = 0; }
            const int64_t m = std::min<int64_t>(64, agents[a].n - j);
            if (!segs.empty() && segs.back().agent == a && segs.back().round == round) segs.back().count += m;
            else segs.push_back(FxItemSegment{(int32_t)a, round, j, m, used});
            used += tile;
        }
    }
    return segs;
}

// The table of such a call: what its kernels and launches need to know of each row -- one row per segment, in the segments'
// order -- and of each round.  per_tile: a row's items per tile of 64 candidates (0: the row runs no item); agents: as given to
// fx_item_rounds, for the scratch share of a row's agent.
//   * a row's nb is its count rounded up to whole tiles; a round's rows are [row0, row0 + n_rows), consecutive and in call order;
//   * item0 / fin0: the row's first item / first finish workgroup in its round's launches, from 0 at the round's first row; a row
//     has (nb / 64) x per_tile items and ceil(count / 256) finish workgroups of 256, and a round has the sums -- so a row without
//     items shares item0 with the row behind it (the kernels' row search finds that one);
//   * scratch: bytes of the largest round, every row's segment whole tiles; agent_row: a row of the agent (its last), -1 without one.
// A round whose items or finish workgroups exceed a launch's 2^31 - 1 is refused.  Pure: no HIP call (tests/item_rounds.cpp).
struct FxItemRound {
    int32_t row0, n_rows;
    int64_t items;          // of all its rows
    int32_t fin_blocks;
};
struct FxItemTable {
    std::vector<int64_t> nb, item0;   // [rows]
    std::vector<int32_t> fin0;        // [rows]
    std::vector<FxItemRound> rounds;
    std::vector<int32_t> agent_row;   // [n_agents]
    size_t scratch = 0;
};
inline int fx_item_table(const std::vector<FxItemSegment> &segs, const FxItemAgent *agents, int n_agents, const int64_t *per_tile,
                         FxItemTable &t) {
    const size_t R = segs.size();
    t = FxItemTable{};
    t.nb.resize(R), t.item0.resize(R), t.fin0.resize(R);
    t.rounds.assign(R ? (size_t)segs.back().round + 1 : 0, FxItemRound{0, 0, 0, 0});
    t.agent_row.assign((size_t)n_agents, -1);
    for (size_t k = 0; k < R; k++) {
        const FxItemSegment &g = segs[k];
        const int64_t tiles = (g.count + 63) / 64;
        FxItemRound &rd = t.rounds[g.round];
        if (rd.n_rows == 0) rd.row0 = (int32_t)k;
        rd.n_rows++;
        t.nb[k] = tiles * 64, t.item0[k] = rd.items, t.fin0[k] = rd.fin_blocks;
        rd.items += tiles * per_tile[k];
        const int64_t fin = (int64_t)rd.fin_blocks + (g.count + 255) / 256;
        if (fin > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld workgroups of candidates", (long long)fin);
        rd.fin_blocks = (int32_t)fin;
        t.scratch = std::max(t.scratch, g.scratch_off + (size_t)t.nb[k] * agents[g.agent].per_candidate_bytes);
        t.agent_row[g.agent] = (int32_t)k;
    }
    for (const FxItemRound &rd : t.rounds)
        if (rd.items > 0x7fffffffLL) return set_err(FX_ERR_CAPACITY, "a round of %lld items", (long long)rd.items);
    return FX_OK;
}

// wait for everything on the context's stream; what stays unknown is what a caller's own stream may hold (FxContext.tail_work)
inline int fx_drain(FxContext *c) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tail_work = c->user_stream;
    return FX_OK;
}

// the resident inputs and outputs are the last evaluation's: no upload (clears `evaluated`) and no state update since
inline bool fx_inputs_current(const FxContext *c) { return c->evaluated && !c->probs_dirty && !(c->dirty_hi > c->dirty_lo); }

// the two refusals of every pass that reads what the last evaluation left; each call site keeps its place among the pass's refusals
inline int fx_check_inputs_current(const FxContext *c) {
    return fx_inputs_current(c) ? FX_OK
                                : set_err(FX_ERR_NOT_READY, "the inputs were rewritten since the last evaluation (fx_update_state): evaluate first");
}
inline int fx_check_not_timed_out(const FxContext *c) {
    return c->timed_out ? set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it") : FX_OK;
}

// Room for a pass's block and, where it has them, its pinned staging buffers `up` and `down`.  All are grow-only, and one that grows
// is freed first: where something that already exists must grow, what was queued on it runs out before -- one wait, in front of the
// first `ensure`; tail_work stays as it is.
inline int fx_pass_room(FxContext *c, FxDeviceBlock &block, size_t bytes, FxPinned<char> *up = nullptr, size_t up_bytes = 0,
                        FxPinned<char> *down = nullptr, size_t down_bytes = 0) {
    if ((block && bytes > block.size()) || (up && *up && up_bytes > up->size()) || (down && *down && down_bytes > down->size()))
        HIP_TRY(hipStreamSynchronize(c->stream));
    FX_TRY(block.ensure(bytes));
    if (up) FX_TRY(up->ensure(up_bytes, hipHostMallocDefault));
    if (down) FX_TRY(down->ensure(down_bytes, hipHostMallocDefault));
    return FX_OK;
}

// Position of the prediction term in an agent's cost list, -1 without one.  Whether a pass sums its costs in the deferred form
// follows from it, but not in one way, so the caller forms that bit: the re-score follows the step (FX_MODE_INT_DEFER_OBST and a
// prediction term: a deferred step without one closed nothing in the obstacle kernel), the hypotheses pass runs the obstacle stage
// itself whatever the step did (a prediction term alone).
inline int fx_prediction_term(const DevProblem &hp) {
    for (int m = 0; m < hp.n_cost; m++)
        if (hp.cost_id[m] == FX_COST_PREDICTION) return m;
    return -1;
}

// a caller's list of n candidates of an agent with C of them: the list is there (fx_check_id_list), every entry is a candidate
// (fx_check_id_range); fx_check_ids is both, for the callers that have nothing to check in between
inline int fx_check_id_list(int64_t n, const int64_t *ids, const char *count_name) {
    return (n < 0 || (n > 0 && !ids)) ? set_err(FX_ERR_INVALID_ARGUMENT, "ids inconsistent (%s=%lld)", count_name, (long long)n) : FX_OK;
}
inline int fx_check_id_range(int64_t n, const int64_t *ids, int64_t C) {
    for (int64_t j = 0; ids && j < n; j++)
        if (ids[j] < 0 || ids[j] >= C) return set_err(FX_ERR_INVALID_ARGUMENT, "candidate %lld out of range", (long long)ids[j]);
    return FX_OK;
}
inline int fx_check_ids(int64_t n, const int64_t *ids, int64_t C, const char *count_name) {
    const int rc = fx_check_id_list(n, ids, count_name);
    return rc ? rc : fx_check_id_range(n, ids, C);
}
