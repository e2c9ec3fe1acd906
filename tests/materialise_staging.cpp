// materialise_staging.cpp -- what fx_materialise_candidates_batch hands to the list launcher for 129
// agents, without a GPU: the library's host sources, malloc-backed fakes of the HIP runtime calls on the way (tests/batch_staging.cpp
// has the same ones) that count every call, launcher stubs that succeed, and a stub of fx_launch_eval_list that keeps what it is
// given (tests/test_materialise_staging.py builds it with the compiler's host pass and runs it).
// A context of 129 agents is created, 129 select-only problems of 20 / 45 / 80 / 320 candidates with K = 0 / 2 / 4 obstacles, every
// fifth with a windowed cost term, are uploaded and "evaluated" through the stubs, and the call is made over all agents and over
// [128, 64, 0, 63, 65], at 1 and at 32 lanes, agent a with a list of 1 + (7 a) mod C ids given descending with its first id twice.
// Checked on what the stub received:
//   * one launch per kernel variant (lanes, obstacle stage, windowed terms) present, four at most, the variants ascending, each
//     launch's rows behind the previous launch's in ONE table, n the longest list and lds the largest need of its rows;
//   * the rows are the listed agents with a list, by variant and within a variant in call order; each clone's C, ld and n_blocks
//     for 256 / G candidates per workgroup, its mode bits, a windowed agent at one lane whatever is set;
//   * every clone's seven output pointers inside ONE live device block, the agent's own, no two agents in the same block; the row
//     table, the clones, the lists and the selection scratch inside ONE other live block;
//   * the uploaded lists ascending and de-duplicated; fx_sparse_view answers with the same list and block;
//   * fx_device_bytes equal to the live device bytes of the fakes' table after every call;
//   * a refused call (an agent listed twice, an id out of range behind valid agents) changes no block and no set;
//   * the fakes' call counter is the same for a second call over 3 agents and a second call over 129.
// Prints "ok" with that count and returns 0, or says what failed and returns 1.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "fx_pass.h"
#include "fx_risk_args.h"
#include "fxplan.h"

// ---- the list launcher: keep what it was given (every other launcher: the stubs of csrc/fx_host_stubs.cpp) ----
struct Launch {
    const DevProblem *prob;
    const int64_t *ids;
    int64_t n;
    size_t lds;
    bool obst, extra;
    const EvalListRow *rows;
    int n_rows, lanes;
    bool ev0, ev1;
};
static std::vector<Launch> g_launches;
extern "C" hipError_t fx_launch_eval_list(const DevProblem *d_prob, const int64_t *d_ids, int64_t n, size_t lds_bytes, bool obst, bool extra,
                                          const EvalListRow *d_rows, int n_rows, int lanes, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t) {
    g_launches.push_back(Launch{d_prob, d_ids, n, lds_bytes, obst, extra, d_rows, n_rows, lanes, ev_start != nullptr, ev_stop != nullptr});
    return hipSuccess;
}

// ---- the fake runtime (tests/batch_staging.cpp), every call counted ----
enum Kind { DEVICE, PINNED, EVENT, STREAM };
struct Block { Kind kind; size_t bytes; int frees; };
static std::map<void *, Block> g_table;   // everything handed out; memory is kept to the end, so no address repeats
static int g_bad_frees = 0;
static long g_calls = 0;
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
// the live device block that holds [p, p + bytes), or null
static const char *block_of(const void *p, size_t bytes) {
    for (auto &b : g_table) {
        const char *base = static_cast<const char *>(b.first), *q = static_cast<const char *>(p);
        if (!b.second.frees && b.second.kind == DEVICE && q >= base && q + bytes <= base + b.second.bytes) return base;
    }
    return nullptr;
}

extern "C" {
hipError_t hipGetDeviceCount(int *count) { g_calls++; *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { g_calls++; return hipSuccess; }
hipError_t hipGetLastError(void) { g_calls++; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { g_calls++; return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { g_calls++; return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamDestroy(hipStream_t s) { g_calls++; return take_back(s, STREAM); }
hipError_t hipStreamSynchronize(hipStream_t) { g_calls++; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { g_calls++; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { g_calls++; return hand_out(reinterpret_cast<void **>(e), 1, EVENT); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { g_calls++; return hand_out(reinterpret_cast<void **>(e), 1, EVENT); }
hipError_t hipEventDestroy(hipEvent_t e) { g_calls++; return take_back(e, EVENT); }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { g_calls++; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { g_calls++; return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { g_calls++; return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { g_calls++; *ms = 0.f; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) { g_calls++; return hand_out(p, bytes, DEVICE); }
hipError_t hipFree(void *p) { g_calls++; return take_back(p, DEVICE); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { g_calls++; return hand_out(p, bytes, PINNED); }
hipError_t hipHostFree(void *p) { g_calls++; return take_back(p, PINNED); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int) { g_calls++; *dev = host; return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { g_calls++; memset(dst, value, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { g_calls++; memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { g_calls++; memcpy(dst, src, bytes); return hipSuccess; }
}

// ---- the checks ----
static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failed++ < 40) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

constexpr int A = 129, N = 10, S = N + 1, M = 8, P = 10;

static int grid_of(int a) { const int g[4] = {2, 3, 4, 8}; return g[a % 4]; }     // 5 g^2 candidates: 20, 45, 80, 320
static int64_t cands(int a) { return 5LL * grid_of(a) * grid_of(a); }
static int obst_K(int a) { return 2 * (a % 3); }                                   // 0 (agents 0, 63, ...), 2, 4
static bool windowed(int a) { return a % 5 == 4; }                                 // (agents 64 and 129 - 5 among them)

// one agent's select-only problem (tests/batch_staging.cpp's, without the bundle and the cost map)
struct Problem {
    std::vector<double> tpow, t, v, d, ref[8], pos, cov, w;
    std::vector<int32_t> npred, ids;
    FxProblem p;
    explicit Problem(int a) {
        const int n = grid_of(a), K = obst_K(a);
        memset(&p, 0, sizeof(p));
        tpow.assign(5 * S, 0.0);
        for (int k = 0; k < 5; k++)
            for (int i = 0; i < S; i++) { tpow[k * S + i] = 1.0; for (int e = 0; e <= k; e++) tpow[k * S + i] *= 0.1 * i; }
        for (int i = 0; i < n; i++) { t.push_back(0.1 * (N - i % N)); v.push_back(8.0 + i); }
        for (int i = 0; i < 5; i++) d.push_back(-0.4 + 0.2 * i);
        for (auto &r : ref) r.assign(M, 0.0);
        for (int k = 0; k < M; k++) { ref[0][k] = ref[4][k] = 5.0 * k; ref[7][k] = 1.0; }
        pos.assign(2 * (size_t)K * P + 2, 30.0); cov.assign(4 * (size_t)K * P + 4, 0.0); npred.assign(K + 1, P);
        for (int j = 0; j < K * P; j++) cov[4 * j] = cov[4 * j + 3] = 1.0;
        if (windowed(a)) { ids = {FX_COST_ACCELERATION, FX_COST_PREDICTION, FX_COST_VELOCITY_OFFSET}; w = {0.3, 0.2, 1.0}; }
        else { ids = {FX_COST_PREDICTION, FX_COST_VELOCITY_OFFSET}; w = {0.2, 1.0}; }
        p.N = N; p.dt = 0.1; p.mode = 0; p.lon_mode = FX_LON_VELOCITY_KEEPING;
        p.x0_lon[1] = 10.0; p.v_des = 10.0;
        p.tpow = tpow.data();
        p.nT = p.nV = n; p.nD = 5; p.t_samp = t.data(); p.v_samp = v.data(); p.d_samp = d.data();
        p.M = M; p.ref_pos = ref[0].data(); p.ref_theta = ref[1].data(); p.ref_curv = ref[2].data(); p.ref_curv_d = ref[3].data();
        p.ref_x = ref[4].data(); p.ref_y = ref[5].data(); p.ref_nx = ref[6].data(); p.ref_ny = ref[7].data();
        p.n_cost = (int)ids.size(); p.cost_id = ids.data(); p.cost_w = w.data();
        p.K = K; p.P = K ? P : 0;
        if (K) { p.obs_pos = pos.data(); p.obs_cov_inv = cov.data(); p.obs_npred = npred.data(); }
    }
};

// agent a's list as the caller gives it: 1 + (7 a) mod C ids from the top of its grid, descending, the first one twice
static std::vector<int64_t> list_of(int a) {
    const int64_t C = cands(a), m = 1 + (7LL * a) % C;
    std::vector<int64_t> l;
    for (int64_t j = 0; j < m; j++) l.push_back(C - 1 - j);
    l.push_back(l[0]);
    return l;
}
static int64_t unique_of(int a) { return 1 + (7LL * a) % cands(a); }

using Variant = std::tuple<int, bool, bool>;
static Variant variant_of(int a, int lanes) { return Variant{windowed(a) ? 1 : lanes, obst_K(a) > 0, windowed(a)}; }

static int call_batch(FxContext *c, const std::vector<int> &listed, const std::vector<std::vector<int64_t>> &lists) {
    std::vector<int32_t> ag(listed.begin(), listed.end());
    std::vector<int64_t> n;
    std::vector<const int64_t *> p;
    for (auto &l : lists) { n.push_back((int64_t)l.size()); p.push_back(l.data()); }
    g_launches.clear();
    return fx_materialise_candidates_batch(c, (int)ag.size(), ag.data(), n.data(), p.data());
}

static void check_call(FxContext *c, const std::vector<int> &listed, int lanes, const char *what) {
    std::vector<std::vector<int64_t>> lists;
    for (int a : listed) lists.push_back(list_of(a));
    CHECK(call_batch(c, listed, lists) == FX_OK, "%s at %d lanes: %s", what, lanes, fx_last_error());
    if (g_failed) return;
    CHECK((size_t)fx_device_bytes(c) == live_device(), "%s: %lld bytes counted, %zu live", what, (long long)fx_device_bytes(c), live_device());
    // the expected rows: by variant, within a variant in call order
    std::vector<int> order(listed);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return variant_of(x, lanes) < variant_of(y, lanes); });
    std::set<Variant> present;
    for (int a : listed) present.insert(variant_of(a, lanes));
    CHECK(g_launches.size() == present.size() && present.size() <= 4, "%s: %zu launches for %zu variants", what, g_launches.size(), present.size());
    int32_t i_lanes = 0, i_launches = 0, i_rows = 0;
    CHECK(fx_last_materialise_info(c, &i_lanes, &i_launches, &i_rows) == FX_OK && i_launches == (int)g_launches.size() && i_rows == (int)listed.size() &&
          i_lanes == std::get<0>(*present.rbegin()), "%s: info says %d lanes, %d launches, %d rows", what, i_lanes, i_launches, i_rows);
    if (g_failed) return;
    size_t row = 0;
    const EvalListRow *table = g_launches[0].rows;
    const char *call_block = block_of(table, sizeof(EvalListRow) * listed.size());
    CHECK(call_block != nullptr, "%s: the row table lies in no live device block", what);
    std::set<const char *> agent_blocks;
    auto vi = present.begin();
    for (size_t k = 0; k < g_launches.size() && !g_failed; k++, ++vi) {
        const Launch &l = g_launches[k];
        CHECK(l.rows == table + row && l.prob == nullptr && l.ids == nullptr, "%s: launch %zu starts at row %td, expected %zu", what, k, l.rows - table, row);
        CHECK(Variant(l.lanes, l.obst, l.extra) == *vi, "%s: launch %zu is (%d, %d, %d)", what, k, l.lanes, (int)l.obst, (int)l.extra);
        CHECK(l.ev0 == (k == 0) && l.ev1 == (k + 1 == g_launches.size()), "%s: launch %zu carries the wrong events", what, k);
        int64_t n_max = 0;
        for (int r = 0; r < l.n_rows && !g_failed; r++, row++) {
            CHECK(row < order.size(), "%s: more rows than listed agents", what);
            if (g_failed) break;
            const int a = order[row];
            CHECK(variant_of(a, lanes) == *vi, "%s: row %zu (agent %d) is in the launch of another variant", what, row, a);
            const EvalListRow &er = l.rows[r];
            CHECK(block_of(er.clone, sizeof(DevProblem)) == call_block, "%s: agent %d: its clone is outside the call's block", what, a);
            if (g_failed) break;
            const DevProblem &d = *er.clone;
            const int64_t m = unique_of(a), ld = (m + 63) / 64 * 64;
            const int cpb = 256 / l.lanes;
            CHECK(d.C == m && d.ld == ld && d.n_blocks == (int)((m + cpb - 1) / cpb), "%s: agent %d: C %lld, ld %lld, n_blocks %d for %lld ids at %d lanes", what, a,
                  (long long)d.C, (long long)d.ld, d.n_blocks, (long long)m, l.lanes);
            CHECK((d.mode & FX_MODE_WRITE_BUNDLE) && (d.mode & FX_MODE_WRITE_COSTMAP) &&
                  !(d.mode & (FX_MODE_INT_DEFER_OBST | FX_MODE_INT_REC_LDS | FX_MODE_INT_STORE_WT)), "%s: agent %d: mode %x", what, a, d.mode);
            CHECK(d.K == obst_K(a) && d.S == S, "%s: agent %d: K %d, S %d in its clone", what, a, d.K, d.S);
            n_max = std::max(n_max, m);
            // the seven outputs in the agent's ONE block, the selection scratch and the list in the call's
            const size_t n_cost = windowed(a) ? 3 : 2;
            const char *b = block_of(d.planes, 8 * (size_t)FX_NUM_PLANES * S * ld);
            CHECK(b != nullptr && b != call_block && block_of(d.coeffs, 8 * (size_t)FX_COEFF_ROWS * ld) == b && block_of(d.traj_len, 4 * (size_t)ld) == b &&
                  block_of(d.costmap, 8 * n_cost * ld) == b && block_of(d.cost, 8 * (size_t)ld) == b && block_of(d.flags, 4 * (size_t)ld) == b &&
                  block_of(d.bound_step, 4 * (size_t)ld) == b, "%s: agent %d: its outputs are not in one live block of its own", what, a);
            CHECK(agent_blocks.insert(b).second, "%s: agent %d shares its block with another agent", what, a);
            CHECK(block_of(d.counters, 8 * FX_CNT_COUNT) == call_block && block_of(d.part_cost, 8 * (size_t)d.n_blocks) == call_block &&
                  block_of(d.part_idx, 8 * (size_t)d.n_blocks) == call_block && block_of(er.ids, 8 * (size_t)m) == call_block,
                  "%s: agent %d: selection scratch or list outside the call's block", what, a);
            if (g_failed) break;
            bool zero = true;
            for (int q = 0; q < FX_CNT_COUNT; q++) zero = zero && d.counters[q] == 0ULL;
            CHECK(zero, "%s: agent %d: counters not cleared", what, a);
            const int64_t C = cands(a);
            bool asc = true;
            for (int64_t j = 0; j < m; j++) asc = asc && er.ids[j] == C - m + j;
            CHECK(asc, "%s: agent %d: the uploaded list is not its ids ascending and de-duplicated", what, a);
            FxSparseView v;
            CHECK(fx_sparse_view(c, a, &v) && v.n == m && v.ld == ld && v.planes == d.planes && v.cost == d.cost && v.ids[0] == C - m, "%s: agent %d: the set's view", what, a);
            CHECK(l.lds >= fx_generic_lds(M, S, 0), "%s: launch %zu: %zu bytes of LDS", what, k, l.lds);
        }
        CHECK(l.n == n_max, "%s: launch %zu: n %lld, its longest list has %lld", what, k, (long long)l.n, (long long)n_max);
    }
    CHECK(row == order.size(), "%s: %zu rows for %zu listed agents", what, row, order.size());
}

static long calls_of(FxContext *c, const std::vector<int> &listed) {
    std::vector<std::vector<int64_t>> lists;
    for (int a : listed) lists.push_back(list_of(a));
    const long before = g_calls;
    CHECK(call_batch(c, listed, lists) == FX_OK, "a repeated call: %s", fx_last_error());
    return g_calls - before;
}

int main() {
    FxContext *c = nullptr;
    int64_t total = 0;
    for (int a = 0; a < A; a++) total += cands(a) + 64;
    CHECK(fx_create_batch(&c, 0, A, total, N, M, 4, P) == FX_OK && c, "create: %s", fx_last_error());
    if (!c) return 1;
    std::vector<Problem> probs;
    probs.reserve(A);
    std::vector<FxProblem> ps;
    for (int a = 0; a < A; a++) { probs.emplace_back(a); ps.push_back(probs.back().p); }
    CHECK(fx_upload_batch(c, A, ps.data()) == FX_OK, "upload: %s", fx_last_error());
    CHECK(fx_evaluate(c) == FX_OK, "evaluate: %s", fx_last_error());
    if (g_failed) return 1;
    const size_t before_any = live_device();
    CHECK(fx_set_materialise_lanes(c, 32) == FX_OK && fx_set_materialise_lanes(c, 1) == FX_OK && live_device() == before_any &&
          (size_t)fx_device_bytes(c) == before_any, "the setting takes device memory");

    std::vector<int> all(A);
    for (int a = 0; a < A; a++) all[a] = a;
    const std::vector<int> some = {128, 64, 0, 63, 65};
    for (int lanes : {1, 32}) {
        CHECK(fx_set_materialise_lanes(c, lanes) == FX_OK, "lanes %d: %s", lanes, fx_last_error());
        check_call(c, all, lanes, "all agents");
        check_call(c, some, lanes, "a list out of order");
        if (g_failed) break;
        // refused calls: no block changes, every set stays
        const size_t live = live_device(), blocks = g_table.size();
        std::vector<std::vector<int64_t>> l3 = {list_of(3), list_of(4), list_of(3)};
        CHECK(call_batch(c, {3, 4, 3}, l3) == FX_ERR_INVALID_ARGUMENT && g_launches.empty(), "an agent listed twice was accepted");
        std::vector<std::vector<int64_t>> l2 = {list_of(3), {0, cands(4)}};
        CHECK(call_batch(c, {3, 4}, l2) == FX_ERR_INVALID_ARGUMENT && g_launches.empty(), "an id equal to C was accepted");
        CHECK(live_device() == live && g_table.size() == blocks && (size_t)fx_device_bytes(c) == live, "a refused call changed a block");
        FxSparseView v;
        for (int a : some) CHECK(fx_sparse_view(c, a, &v) && v.n == unique_of(a), "agent %d lost its set to a refused call", a);
    }
    // the runtime calls of a call do not depend on the agent count once the blocks have grown
    long n3 = 0, n129 = 0;
    if (!g_failed) {
        calls_of(c, all);
        n129 = calls_of(c, all);
        calls_of(c, {5, 6, 7});
        n3 = calls_of(c, {5, 6, 7});     // (5, 6 and 7 take the same variants as all agents do: launches alike)
        CHECK(n3 == n129 && n3 > 0, "%ld runtime calls for 3 agents, %ld for 129", n3, n129);
    }
    CHECK(fx_destroy(c) == FX_OK && g_bad_frees == 0, "destroy: %d bad frees", g_bad_frees);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok (%d agents, %ld runtime calls per repeated call)\n", A, n3);
    return 0;
}
