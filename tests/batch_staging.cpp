// batch_staging.cpp -- what the four batched entries beside the plan step (fx_eval_prediction_prob_batch,
// fx_eval_responsibility_cost_batch, fx_eval_risk_batch, fx_eval_risk_costs_batch; DESIGN.md sections 18-21) hand to their
// launchers for 129 agents, without a GPU: the library's host sources, malloc-backed fakes of the HIP runtime calls on the way
// (tests/context_owners.cpp has the same ones for create and upload), launcher stubs that succeed, and stubs of the four batched
// launchers that keep their argument (tests/test_batch_staging.py builds it with the compiler's host pass and runs it).
// A context of 129 agents is created, 129 problems of 20 / 45 / 80 / 320 candidates are uploaded and "evaluated" through the
// stubs, every agent gets K = 0 / 2 / 4 risk obstacles (agents 0 and 63: none), and each entry is called over all agents -- at
// the library's scratch limit: one round -- and over a list given out of order.  Checked on what the stub received:
//   * agent_row[] has A entries: the agent's row, or -1 for an agent with an empty list; the rows are in call order, one per
//     agent with candidates, with the agent's own n, first = 0 and count = n;
//   * item0[] / fin0[] are the compact copies of the rows' fields, ascend, start at 0 and advance by the row's own
//     (nb / 64) x chunks x K items and ceil(count / 256) workgroups; a row of an agent without obstacles has no item and shares
//     item0 with the row behind it; the round's sums are the launch sizes;
//   * blk0[] has one entry per agent (the responsibility pass) or per agent WITH cost parameters (the cost pass, compact, in
//     call order): the running sum of ceil(n / 256), `blocks` the total; cost[] / sum[] at the same index are that agent's;
//   * seg_blk0[] has 4 A entries: the running sum of ceil(K n / 1024), plane q of agent i at 4 i + q, its source in the agent's
//     column block and its destination in column q of the call;
//   * every table, every row's scratch, outputs and columns lie inside ONE live device block of the fake runtime, and
//     fx_device_bytes equals the live device bytes of the fakes' table after every call.
// Prints "ok" and returns 0, or says what failed and returns 1.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "fx_pass.h"
#include "fx_risk_args.h"
#include "fxplan.h"

// ---- the four batched launchers: keep what they were given (every other launcher: the stubs of csrc/fx_host_stubs.cpp) ----
static PredProbBatchArgs g_pp;
static RiskBatchArgs g_resp;
static RiskListBatchArgs g_list;
static RiskCostBatchArgs g_cost;
static std::vector<FxItemRound> g_rounds;
static int g_launches = 0;
static void keep_rounds(const FxItemRound *rounds, int n) { g_rounds.assign(rounds, rounds + n); g_launches++; }
extern "C" {
hipError_t fx_launch_predprob_batch(const PredProbBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *, hipEvent_t, hipEvent_t,
                                    hipStream_t) { g_pp = *t; keep_rounds(rounds, n_rounds); return hipSuccess; }
hipError_t fx_launch_risk_batch(const RiskBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *, hipEvent_t, hipEvent_t,
                                hipStream_t) { g_resp = *t; keep_rounds(rounds, n_rounds); return hipSuccess; }
hipError_t fx_launch_risk_list_batch(const RiskListBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *, hipEvent_t, hipEvent_t,
                                     hipStream_t) { g_list = *t; keep_rounds(rounds, n_rounds); return hipSuccess; }
hipError_t fx_launch_risk_costs_batch(const RiskCostBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *, long long *, hipEvent_t,
                                      hipEvent_t, hipStream_t) { g_cost = *t; keep_rounds(rounds, n_rounds); return hipSuccess; }
}

// ---- the fake runtime (tests/context_owners.cpp), with the calls an evaluation and a pass beside it make ----
enum Kind { DEVICE, PINNED, EVENT, STREAM };
struct Block { Kind kind; size_t bytes; int frees; };
static std::map<void *, Block> g_table;   // everything handed out; memory is kept to the end, so no address repeats
static int g_bad_frees = 0;
static hipError_t hand_out(void **p, size_t bytes, Kind kind) {
    *p = calloc(bytes ? bytes : 1, 1);
    g_table[*p] = Block{kind, bytes, 0};
    return hipSuccess;
}
static hipError_t take_back(void *p, Kind kind) {
    auto it = g_table.find(p);
    if (it == g_table.end() || it->second.kind != kind || it->second.frees++) { g_bad_frees++; return hipErrorInvalidValue; }
    return hipSuccess;
}
static size_t live_device() {
    size_t n = 0;
    for (auto &b : g_table)
        if (!b.second.frees && b.second.kind == DEVICE) n += b.second.bytes;
    return n;
}
// the live device block that holds p, or null
static const char *block_of(const void *p, size_t *bytes) {
    for (auto &b : g_table) {
        const char *base = static_cast<const char *>(b.first);
        if (!b.second.frees && b.second.kind == DEVICE && static_cast<const char *>(p) >= base && static_cast<const char *>(p) < base + b.second.bytes) {
            *bytes = b.second.bytes;
            return base;
        }
    }
    return nullptr;
}

extern "C" {
hipError_t hipGetDeviceCount(int *count) { *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamDestroy(hipStream_t s) { return take_back(s, STREAM); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { return hand_out(reinterpret_cast<void **>(e), 1, EVENT); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hand_out(reinterpret_cast<void **>(e), 1, EVENT); }
hipError_t hipEventDestroy(hipEvent_t e) { return take_back(e, EVENT); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) { return hand_out(p, bytes, DEVICE); }
hipError_t hipFree(void *p) { return take_back(p, DEVICE); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return hand_out(p, bytes, PINNED); }
hipError_t hipHostFree(void *p) { return take_back(p, PINNED); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int) { *dev = host; return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { memset(dst, value, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
}

// ---- the checks ----
static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 40) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

constexpr int A = 129, N = 10, S = N + 1, M = 8, KO = 2, P = 10;

static int grid_of(int a) { const int g[4] = {2, 3, 4, 8}; return g[a % 4]; }     // 5 g^2 candidates: 20, 45, 80, 320
static int64_t cands(int a) { return 5LL * grid_of(a) * grid_of(a); }
static int risk_K(int a) { return 2 * (a % 3); }                                   // 0 (agents 0, 63, ...), 2, 4

// one agent's problem (tests/context_owners.cpp) with the bundle, the cost map and a cost list with the prediction in it
struct Problem {
    std::vector<double> tpow, t, v, d, ref[8], pos, cov, w;
    std::vector<int32_t> npred, ids;
    FxProblem p;
    explicit Problem(int n) {
        memset(&p, 0, sizeof(p));
        tpow.assign(5 * S, 0.0);
        for (int k = 0; k < 5; k++)
            for (int i = 0; i < S; i++) { tpow[k * S + i] = 1.0; for (int e = 0; e <= k; e++) tpow[k * S + i] *= 0.1 * i; }
        for (int i = 0; i < n; i++) { t.push_back(0.1 * (N - i % N)); v.push_back(8.0 + i); }
        for (int i = 0; i < 5; i++) d.push_back(-0.4 + 0.2 * i);
        for (auto &r : ref) r.assign(M, 0.0);
        for (int k = 0; k < M; k++) { ref[0][k] = ref[4][k] = 5.0 * k; ref[7][k] = 1.0; }
        pos.assign(2 * KO * P, 30.0); cov.assign(4 * KO * P, 0.0); npred.assign(KO, P);
        for (int j = 0; j < KO * P; j++) cov[4 * j] = cov[4 * j + 3] = 1.0;
        ids = {FX_COST_PREDICTION, FX_COST_VELOCITY_OFFSET};
        if (ids[0] > ids[1]) std::swap(ids[0], ids[1]);
        w = {0.2, 1.0};
        p.N = N; p.dt = 0.1; p.mode = FX_MODE_WRITE_BUNDLE | FX_MODE_WRITE_COSTMAP; p.lon_mode = FX_LON_VELOCITY_KEEPING;
        p.x0_lon[1] = 10.0; p.v_des = 10.0;
        p.tpow = tpow.data();
        p.nT = p.nV = n; p.nD = 5; p.t_samp = t.data(); p.v_samp = v.data(); p.d_samp = d.data();
        p.M = M; p.ref_pos = ref[0].data(); p.ref_theta = ref[1].data(); p.ref_curv = ref[2].data(); p.ref_curv_d = ref[3].data();
        p.ref_x = ref[4].data(); p.ref_y = ref[5].data(); p.ref_nx = ref[6].data(); p.ref_ny = ref[7].data();
        p.n_cost = 2; p.cost_id = ids.data(); p.cost_w = w.data();
        p.K = KO; p.P = P; p.obs_pos = pos.data(); p.obs_cov_inv = cov.data(); p.obs_npred = npred.data();
    }
};

static FxRiskParams risk_params(int a) {
    FxRiskParams p;
    memset(&p, 0, sizeof(p));
    p.prob_mode = FX_RISK_PROB_MVN;
    p.prot_model = p.unprot_ego_model = FX_RISK_HARM_LOGISTIC;
    p.ego_length = 4.5 + 0.01 * a; p.ego_width = 1.6; p.ego_mass = 1200.0 + a;
    return p;
}

static void set_tables(FxContext *c, int a) {
    const int K = risk_K(a);
    std::vector<double> pos(2 * (size_t)K * P, 1.0), cov(4 * (size_t)K * P, 0.0), yaw((size_t)K * P, 0.0), v((size_t)K * P, 1.0), len(K, 4.0),
        wid(K, 1.8), mass(K, 1000.0);
    for (size_t j = 0; j < (size_t)K * P; j++) cov[4 * j] = cov[4 * j + 3] = 1.0;
    std::vector<int32_t> n(K, P), cls(K, FX_RISK_CLASS_PROTECTED);
    const int rc = fx_set_risk_obstacles_agent(c, a, K, P, pos.data(), cov.data(), cov.data(), yaw.data(), v.data(), n.data(), n.data(), n.data(),
                                               len.data(), wid.data(), mass.data(), cls.data());
    CHECK(rc == FX_OK, "tables of agent %d: %s", a, fx_last_error());
}

// [p, p + bytes) lies in the block [base, base + size)
static bool inside(const void *p, size_t bytes, const char *base, size_t size) {
    const char *q = static_cast<const char *>(p);
    return q >= base && q + bytes <= base + size;
}

// what the four calls share: the table of `listed` agents with n[i] list positions (or candidates) each, one round
template <class Row, class RowK>
static void check_table(const char *what, FxContext *c, const BatchTable<Row> &t, const std::vector<int> &listed, const std::vector<int64_t> &n,
                        RowK row_fields, const char **base_out, size_t *size_out) {
    const size_t L = listed.size();
    CHECK((size_t)fx_device_bytes(c) == live_device(), "%s: %lld bytes counted, %zu live", what, (long long)fx_device_bytes(c), live_device());
    size_t size = 0;
    const char *base = block_of(t.rows, &size);
    *base_out = base, *size_out = size;
    CHECK(base != nullptr, "%s: the row table lies in no live device block", what);
    if (!base) return;
    size_t n_rows = 0;
    for (size_t i = 0; i < L; i++) n_rows += n[i] > 0;
    CHECK(t.n_agents == (int)L, "%s: n_agents %d of %zu", what, t.n_agents, L);
    CHECK(g_rounds.size() == 1 && g_rounds[0].row0 == 0 && g_rounds[0].n_rows == (int)n_rows, "%s: %zu rounds, %d rows of %zu", what,
          g_rounds.size(), g_rounds.empty() ? -1 : g_rounds[0].n_rows, n_rows);
    CHECK(inside(t.rows, sizeof(Row) * n_rows, base, size) && inside(t.item0, 8 * n_rows, base, size) && inside(t.fin0, 4 * n_rows, base, size) &&
          inside(t.agent_row, 4 * L, base, size), "%s: a table leaves the block of %zu bytes", what, size);
    if (g_failed) return;
    int64_t item_at = 0, fin_at = 0;
    size_t row = 0;
    for (size_t i = 0; i < L; i++) {
        if (n[i] == 0) {
            CHECK(t.agent_row[i] == -1, "%s: agent_row[%zu] = %d for an agent without a row", what, i, t.agent_row[i]);
            continue;
        }
        CHECK(t.agent_row[i] == (int)row, "%s: agent_row[%zu] = %d, its row is %zu", what, i, t.agent_row[i], row);
        const Row &r = t.rows[row];
        int64_t row_n, nb, items;
        row_fields(r, listed[i], row_n, nb, items, base, size);
        CHECK(row_n == n[i] && r.first == 0 && r.count == n[i] && nb == (n[i] + 63) / 64 * 64, "%s: row %zu (agent %d): n %lld, first %lld, count %lld, nb %lld "
              "for %lld", what, row, listed[i], (long long)row_n, (long long)r.first, (long long)r.count, (long long)nb, (long long)n[i]);
        CHECK(r.item0 == item_at && t.item0[row] == item_at && r.fin0 == fin_at && t.fin0[row] == fin_at, "%s: row %zu: item0 %lld / %lld, fin0 %d / %d, "
              "expected %lld, %lld", what, row, (long long)r.item0, (long long)t.item0[row], r.fin0, t.fin0[row], (long long)item_at, (long long)fin_at);
        CHECK((items == 0) == (risk_K(listed[i]) == 0), "%s: row %zu (agent %d, K = %d) has %lld items", what, row, listed[i], risk_K(listed[i]), (long long)items);
        item_at += items;
        fin_at += (n[i] + 255) / 256;
        row++;
    }
    CHECK(g_rounds[0].items == item_at && g_rounds[0].fin_blocks == fin_at, "%s: the round has %lld items, %d finish workgroups; the rows %lld, %lld", what,
          (long long)g_rounds[0].items, g_rounds[0].fin_blocks, (long long)item_at, (long long)fin_at);
}

// the fields of a RiskBatchRow that check_table asks for, and where its pointers lie; nv: partials per (obstacle, chunk)
static auto risk_row(const char *what, int nv, bool with_col) {
    return [=](const RiskBatchRow &r, int agent, int64_t &row_n, int64_t &nb, int64_t &items, const char *base, size_t size) {
        row_n = r.w.n, nb = r.it.nb;
        const int K = risk_K(agent);
        CHECK(r.w.K == K && r.w.S == S, "%s: agent %d: K %d, S %d in its row", what, agent, r.w.K, r.w.S);
        items = K ? nb / 64 * r.it.chunks * K : 0;
        CHECK((r.items != 0) == (K != 0), "%s: agent %d: items %d with K = %d", what, agent, r.items, K);
        CHECK(!K || (r.it.chunks >= 1 && r.it.cs >= 1 && (int64_t)r.it.cs * r.it.chunks >= S - 1), "%s: agent %d: %d chunks of %d steps", what, agent,
              r.it.chunks, r.it.cs);
        const size_t part = 8 * (size_t)nv * K * (K ? r.it.chunks : 0) * (size_t)nb;
        CHECK(inside(r.it.params, sizeof(FxRiskParams), base, size) && (!part || inside(r.it.part, part, base, size)) &&
              inside(r.ego, 8 * (size_t)row_n, base, size) && inside(r.obst, 8 * (size_t)row_n, base, size),
              "%s: agent %d: parameters, partials (%zu bytes) or outputs leave the block", what, agent, part);
        if (with_col)
            CHECK(inside(r.occ, 8 * (size_t)row_n, base, size) && (!K || inside(r.col, 8 * 4 * (size_t)K * row_n, base, size)), "%s: agent %d: columns leave the block",
                  what, agent);
        CHECK(!r.w.ids || inside(r.w.ids, 8 * (size_t)row_n, base, size), "%s: agent %d: its list leaves the block", what, agent);
    };
}

int main() {
    FxContext *c = nullptr;
    int64_t total = 0;
    for (int a = 0; a < A; a++) total += cands(a) + 64;
    CHECK(fx_create_batch(&c, 0, A, total, N, M, KO, P) == FX_OK && c, "create: %s", fx_last_error());
    if (!c) return 1;
    std::vector<Problem> probs;
    probs.reserve(A);
    std::vector<FxProblem> ps;
    for (int a = 0; a < A; a++) { probs.emplace_back(grid_of(a)); ps.push_back(probs.back().p); }
    CHECK(fx_upload_batch(c, A, ps.data()) == FX_OK, "upload: %s", fx_last_error());
    CHECK(fx_evaluate(c) == FX_OK, "evaluate: %s", fx_last_error());
    if (g_failed) return 1;
    for (int a = 0; a < A; a++) set_tables(c, a);

    std::vector<FxRiskParams> prm;
    for (int a = 0; a < A; a++) prm.push_back(risk_params(a));
    std::vector<int> all(A);
    for (int a = 0; a < A; a++) all[a] = a;
    const std::vector<int> some = {128, 64, 0, 63, 65, 127};
    std::vector<double> ones(8, 1.0);
    const char *base;
    size_t size;

    for (const std::vector<int> &listed : {all, some}) {
        const size_t L = listed.size();
        std::vector<int32_t> ag(listed.begin(), listed.end());
        std::vector<FxRiskParams> lp;
        std::vector<int64_t> nC;
        size_t rows = 0, cols = 0;
        for (int a : listed) { lp.push_back(prm[a]); nC.push_back(cands(a)); rows += cands(a); cols += (size_t)risk_K(a) * cands(a); }
        std::vector<double> o[14];
        for (auto &x : o) x.assign(std::max(rows, cols) + 1, 0.0);
        std::vector<int64_t> bi(L), ci(L);
        std::vector<double> bc(L);
        const char *what = L == (size_t)A ? "all agents" : "a list out of order";

        // section 18
        std::vector<FxPredProbParams> pp(L, FxPredProbParams{4.5, 1.6, FX_PRED_SOURCE_PROBABILITY});
        FxPredProbBatchOutputs po{o[0].data(), o[1].data(), bi.data(), bc.data()};
        int before = g_launches;
        CHECK(fx_eval_prediction_prob_batch(c, (int)L, ag.data(), pp.data(), &po) == FX_OK && g_launches == before + 1, "%s: probability: %s", what, fx_last_error());
        check_table("probability", c, g_pp, listed, nC, [&](const PredProbRow &r, int agent, int64_t &row_n, int64_t &nb, int64_t &items, const char *b, size_t sz) {
            row_n = r.a.n, nb = r.a.nb;
            const int K = risk_K(agent);
            CHECK(r.a.K == K && r.a.S == S, "probability: agent %d: K %d, S %d in its row", agent, r.a.K, r.a.S);
            items = K ? nb / 64 * r.chunks * K : 0;
            CHECK(!K || (r.chunks >= 1 && (int64_t)r.cs * r.chunks >= S - 1), "probability: agent %d: %d chunks of %d steps", agent, r.chunks, r.cs);
            CHECK((!K || inside(r.a.step, 8 * (size_t)K * (S - 1) * nb, b, sz)) && inside(r.a.prob, 8 * (size_t)row_n, b, sz) && inside(r.a.total, 8 * (size_t)row_n, b, sz),
                  "probability: agent %d: scratch or outputs leave the block", agent);
        }, &base, &size);

        // section 19: blk0 by agent
        std::vector<FxRespCostParams> rp(L, FxRespCostParams{0.5, FX_RISK_RESP_ACTION_SPACE, ones.data(), nullptr});
        FxRespCostBatchOutputs ro{o[0].data(), o[1].data(), o[2].data(), o[3].data(), bi.data(), bc.data()};
        before = g_launches;
        CHECK(fx_eval_responsibility_cost_batch(c, (int)L, ag.data(), lp.data(), rp.data(), &ro) == FX_OK && g_launches == before + 1, "%s: responsibility: %s", what,
              fx_last_error());
        check_table("responsibility", c, g_resp.t, listed, nC, risk_row("responsibility", 7, true), &base, &size);
        if (base && !g_failed) {
            CHECK(inside(g_resp.blk0, 4 * L, base, size) && inside(g_resp.cost, sizeof(RiskCostArgs) * L, base, size) && inside(g_resp.sum, sizeof(RespSumArgs) * L, base, size),
                  "responsibility: blk0, cost or sum leave the block");
            int64_t at = 0;
            for (size_t i = 0; i < L; i++) {
                CHECK(g_resp.blk0[i] == at, "responsibility: blk0[%zu] = %d, expected %lld", i, g_resp.blk0[i], (long long)at);
                CHECK(g_resp.cost[i].n == nC[i] && g_resp.sum[i].n == nC[i] && g_resp.cost[i].K == risk_K(listed[i]), "responsibility: cost[%zu] / sum[%zu] are not agent %d's",
                      i, i, listed[i]);
                CHECK(inside(g_resp.cost[i].out, 8 * 7 * (size_t)nC[i], base, size) && inside(g_resp.sum[i].total, 8 * (size_t)nC[i], base, size),
                      "responsibility: agent %d: cost rows or totals leave the block", listed[i]);
                at += (nC[i] + 255) / 256;
            }
            CHECK(g_resp.blocks == at && at > (int64_t)L, "responsibility: %d blocks, expected %lld", g_resp.blocks, (long long)at);
        }

        // the list forms of sections 20 and 21, by agent: none / one id / an empty list / every candidate, descending
        std::vector<std::vector<int64_t>> lists(L);
        std::vector<int64_t> n_ids(L), nL(L);
        std::vector<const int64_t *> idp(L);
        static const int64_t none_yet = 0;
        for (size_t i = 0; i < L; i++) {
            const int a = listed[i], form = a % 4 == 3 ? (a / 4) % 4 : a % 4;      // (the agents of 320 candidates take every form in turn)
            if (form == 1) lists[i] = {cands(a) / 2};
            if (form == 3) for (int64_t j = cands(a); j-- > 0;) lists[i].push_back(j);
            n_ids[i] = (int64_t)lists[i].size();
            idp[i] = form == 0 ? nullptr : (lists[i].empty() ? &none_yet : lists[i].data());
            nL[i] = form == 0 ? cands(a) : n_ids[i];
        }

        // section 20
        FxRiskBatchOutputs lo{o[0].data(), o[1].data(), bi.data()};
        before = g_launches;
        CHECK(fx_eval_risk_batch(c, (int)L, ag.data(), lp.data(), n_ids.data(), idp.data(), &lo) == FX_OK && g_launches == before + 1, "%s: risk: %s", what, fx_last_error());
        check_table("risk", c, g_list, listed, nL, risk_row("risk", 2, false), &base, &size);

        // section 21: blk0 compact over the agents with cost parameters, seg_blk0 four per agent
        std::vector<FxRiskCostParams> cps(L);
        std::vector<const FxRiskCostParams *> cpp(L, nullptr);
        std::vector<int> with_cost;
        for (size_t i = 0; i < L; i++) {
            memset(&cps[i], 0, sizeof(cps[i]));
            cps[i].weights[0] = cps[i].weights[4] = 1.0; cps[i].maximin_eps = 1e-9; cps[i].maximin_scale = 10.0;
            cps[i].responsibility_mode = FX_RISK_RESP_ACTION_SPACE; cps[i].responsibility = ones.data();
            if (listed[i] % 3 == 0) continue;      // (two agents of three, 86 of 129: the compact table is longer than a wave too)
            cpp[i] = &cps[i];
            with_cost.push_back((int)i);
        }
        FxRiskCostBatchOutputs co;
        double **fields = reinterpret_cast<double **>(&co);
        for (int k = 0; k < 14; k++) fields[k] = o[k].data();
        co.min_risk_index = bi.data(), co.min_cost_index = ci.data();
        before = g_launches;
        CHECK(fx_eval_risk_costs_batch(c, (int)L, ag.data(), lp.data(), cpp.data(), n_ids.data(), idp.data(), &co) == FX_OK && g_launches == before + 1, "%s: risk costs: %s",
              what, fx_last_error());
        check_table("risk costs", c, g_cost.t, listed, nL, risk_row("risk costs", 7, true), &base, &size);
        if (base && !g_failed) {
            const size_t NC = with_cost.size();
            CHECK(g_cost.n_cost == (int)NC && NC > 0 && NC < L, "risk costs: n_cost %d, %zu agents have cost parameters", g_cost.n_cost, NC);
            CHECK(inside(g_cost.blk0, 4 * NC, base, size) && inside(g_cost.cost, sizeof(RiskCostArgs) * NC, base, size), "risk costs: blk0 or cost leave the block");
            int64_t at = 0;
            for (size_t k = 0; k < NC; k++) {
                const size_t i = (size_t)with_cost[k];
                CHECK(g_cost.blk0[k] == at, "risk costs: blk0[%zu] = %d, expected %lld (agent %d)", k, g_cost.blk0[k], (long long)at, listed[i]);
                CHECK(g_cost.cost[k].n == nL[i] && g_cost.cost[k].K == risk_K(listed[i]) && (nL[i] == 0 || (g_cost.cost[k].ids != nullptr) == (idp[i] != nullptr)),
                      "risk costs: cost[%zu] is not agent %d's", k, listed[i]);
                CHECK(!nL[i] || inside(g_cost.cost[k].out, 8 * 7 * (size_t)nL[i], base, size), "risk costs: agent %d: cost rows leave the block", listed[i]);
                at += (nL[i] + 255) / 256;
            }
            CHECK(g_cost.blocks == at, "risk costs: %d blocks, expected %lld", g_cost.blocks, (long long)at);
            CHECK(g_cost.n_seg == 4 * (int)L && inside(g_cost.seg_blk0, 4 * 4 * L, base, size) && inside(g_cost.seg, sizeof(RiskCopySeg) * 4 * L, base, size),
                  "risk costs: %d segments for %zu agents, or their tables leave the block", g_cost.n_seg, L);
            int64_t seg_at = 0;
            bool big_seg = false;
            size_t T = 0, col_at = 0;
            for (size_t i = 0; i < L; i++) T += (size_t)risk_K(listed[i]) * (size_t)nL[i];
            for (size_t i = 0; i < L && g_cost.n_seg == 4 * (int)L; i++) {
                const size_t Kn = (size_t)risk_K(listed[i]) * (size_t)nL[i];
                for (int q = 0; q < 4; q++) {
                    const RiskCopySeg &g = g_cost.seg[4 * i + q];
                    CHECK(g_cost.seg_blk0[4 * i + q] == seg_at && g.n == (int64_t)Kn, "risk costs: seg_blk0[%zu] = %d (n %lld), expected %lld (n %zu)", 4 * i + q,
                          g_cost.seg_blk0[4 * i + q], (long long)g.n, (long long)seg_at, Kn);
                    CHECK(!Kn || (inside(g.src, 8 * Kn, base, size) && inside(g.dst, 8 * Kn, base, size)), "risk costs: segment %zu leaves the block", 4 * i + q);
                    // plane q of the agent's [4][K][n] block into the agent's place in column q of the call
                    CHECK(!Kn || (g.src - g_cost.seg[4 * i].src == (ptrdiff_t)(q * Kn) && g.dst - g_cost.seg[0].dst == (ptrdiff_t)(q * T + col_at)),
                          "risk costs: segment %zu copies from or to another place", 4 * i + q);
                    seg_at += ((int64_t)Kn + 1023) / 1024;
                    big_seg = big_seg || Kn > 1024;
                }
                col_at += Kn;
            }
            CHECK(g_cost.seg_blocks == seg_at, "risk costs: %d column workgroups, expected %lld", g_cost.seg_blocks, (long long)seg_at);
            if (L == (size_t)A) CHECK(big_seg, "risk costs: no segment of more than one workgroup");
        }
        CHECK((size_t)fx_device_bytes(c) == live_device(), "%s: %lld bytes counted, %zu live", what, (long long)fx_device_bytes(c), live_device());
    }
    CHECK(fx_destroy(c) == FX_OK && g_bad_frees == 0, "destroy: %d bad frees", g_bad_frees);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok (%d agents, %d batched launches)\n", A, g_launches);
    return 0;
}
