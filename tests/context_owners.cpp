// context_owners.cpp -- the context's memory behind its owner types (csrc/fx_owner.h), without a GPU: the library's host sources,
// launcher stubs that succeed (csrc/fx_host_stubs.cpp), and malloc-backed fakes of the HIP runtime entry points that create, upload
// and destroy call (tests/test_context_owners.py builds it with the compiler's host pass and runs it; the definitions here take
// precedence over the runtime library's).  The fakes keep a table of everything handed out -- kind, bytes, frees per pointer -- and can fail the
// k-th call.  Checked:
//   1. create with one and with four agents, destroy: nothing live, every block freed exactly once;
//   2. create with call k failing, for every k of a create: an error, *out == NULL, nothing live;
//   3. uploads across every grow site (planes, boundary pair, obstacle scratch): fx_device_bytes equals the live device bytes of
//      the table after every upload, and nothing is live after destroy.
// The gather block of the survivor exchange needs an RCCL communicator and is not reached here.
// Prints "ok" and returns 0, or says what failed and returns 1.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "fxplan.h"

// ---- the fake runtime ----
enum Kind { DEVICE, PINNED, EVENT, STREAM };
struct Block { Kind kind; size_t bytes; int frees; };
static std::map<void *, Block> g_table;   // everything handed out since reset(); memory is kept until then, so no address repeats
static long g_calls = 0, g_fail_at = 0;   // fallible calls so far; the one to fail (0: none)
static int g_bad_frees = 0;               // frees of something never handed out, of the wrong kind, or a second time

static void reset(long fail_at) {
    for (auto &b : g_table) free(b.first);
    g_table.clear();
    g_calls = 0; g_fail_at = fail_at; g_bad_frees = 0;
}
static bool failing() { return ++g_calls == g_fail_at; }
static hipError_t hand_out(void **p, size_t bytes, Kind kind) {
    if (failing()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_table[*p] = Block{kind, bytes, 0};
    return hipSuccess;
}
static hipError_t take_back(void *p, Kind kind) {
    auto it = g_table.find(p);
    if (it == g_table.end() || it->second.kind != kind || it->second.frees++) { g_bad_frees++; return hipErrorInvalidValue; }
    return hipSuccess;
}
static size_t live(int kind = -1) {   // bytes of a kind, or the number of live entries of all kinds
    size_t n = 0;
    for (auto &b : g_table)
        if (!b.second.frees && (kind < 0 || b.second.kind == kind)) n += kind < 0 ? 1 : b.second.bytes;
    return n;
}

extern "C" {
hipError_t hipGetDeviceCount(int *count) { if (failing()) return hipErrorNoDevice; *count = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return failing() ? hipErrorInvalidDevice : hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int, int) { return hand_out(reinterpret_cast<void **>(s), 1, STREAM); }
hipError_t hipStreamDestroy(hipStream_t s) { return take_back(s, STREAM); }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { return hand_out(reinterpret_cast<void **>(e), 1, EVENT); }
hipError_t hipEventDestroy(hipEvent_t e) { return take_back(e, EVENT); }
hipError_t hipMalloc(void **p, size_t bytes) { return hand_out(p, bytes, DEVICE); }
hipError_t hipFree(void *p) { return take_back(p, DEVICE); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return hand_out(p, bytes, PINNED); }
hipError_t hipHostFree(void *p) { return take_back(p, PINNED); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int) { if (failing()) return hipErrorInvalidValue; *dev = host; return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { if (failing()) return hipErrorInvalidValue; memset(dst, value, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { if (failing()) return hipErrorInvalidValue; memcpy(dst, src, bytes); return hipSuccess; }
}

// ---- the checks ----
static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed++; printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

constexpr int N = 10, S = N + 1, M = 8, K = 2, P = 10;

static int create(FxContext **out, int agents) { return fx_create_batch(out, 0, agents, 256, N, M, K, P); }

static void nothing_left(const char *what) {
    CHECK(live() == 0, "%s: %zu entries still live", what, live());
    CHECK(g_bad_frees == 0, "%s: %d frees of something not held", what, g_bad_frees);
}

// one agent's problem: an n x n x 5 grid of N steps on a straight reference, K obstacles, optionally n_bound boundary pieces
struct Problem {
    std::vector<double> tpow, t, v, d, ref[8], pos, cov, piece;
    std::vector<int32_t> npred, bin, item;
    FxProblem p;
    Problem(int n, uint32_t mode, int n_bound) {
        memset(&p, 0, sizeof(p));
        tpow.assign(5 * S, 0.0);
        for (int k = 0; k < 5; k++)
            for (int i = 0; i < S; i++) { tpow[k * S + i] = 1.0; for (int e = 0; e <= k; e++) tpow[k * S + i] *= 0.1 * i; }
        for (int i = 0; i < n; i++) { t.push_back(0.1 * (N - i)); v.push_back(8.0 + i); }
        for (int i = 0; i < 5; i++) d.push_back(-0.4 + 0.2 * i);
        for (auto &r : ref) r.assign(M, 0.0);
        for (int k = 0; k < M; k++) { ref[0][k] = ref[4][k] = 5.0 * k; ref[7][k] = 1.0; }   // pos, x; normal (0, 1)
        pos.assign(2 * K * P, 30.0); cov.assign(4 * K * P, 0.0); npred.assign(K, P);
        for (int j = 0; j < K * P; j++) cov[4 * j] = cov[4 * j + 3] = 1.0;
        p.N = N; p.dt = 0.1; p.mode = mode; p.lon_mode = FX_LON_VELOCITY_KEEPING; p.x0_lon[1] = 10.0; p.v_des = 10.0;
        p.tpow = tpow.data();
        p.nT = p.nV = n; p.nD = 5; p.t_samp = t.data(); p.v_samp = v.data(); p.d_samp = d.data();
        p.M = M; p.ref_pos = ref[0].data(); p.ref_theta = ref[1].data(); p.ref_curv = ref[2].data(); p.ref_curv_d = ref[3].data();
        p.ref_x = ref[4].data(); p.ref_y = ref[5].data(); p.ref_nx = ref[6].data(); p.ref_ny = ref[7].data();
        p.K = K; p.P = P; p.obs_pos = pos.data(); p.obs_cov_inv = cov.data(); p.obs_npred = npred.data();
        if (n_bound) {   // every piece listed once, all in the first bin
            piece.assign(4 * (size_t)n_bound, 1.0); bin.assign(M + 1, n_bound); bin[0] = 0;
            for (int j = 0; j < n_bound; j++) item.push_back(j);
            p.n_bound = n_bound; p.bound_piece = piece.data(); p.bound_bin = bin.data(); p.bound_item = item.data(); p.bound_d_reach = 3.0;
        }
    }
};

// small, larger, small again on one context; the account equals the table after every upload
static void uploads(const char *what, uint32_t mode, int obstacle_stage, int n_bound_small, int n_bound_large) {
    reset(0);
    FxContext *c = nullptr;
    CHECK(create(&c, 2) == FX_OK && c, "%s: create: %s", what, fx_last_error());
    if (!c) return;
    CHECK(fx_set_obstacle_stage(c, obstacle_stage, 0) == FX_OK, "%s: %s", what, fx_last_error());
    CHECK((size_t)fx_device_bytes(c) == live(DEVICE), "%s: after create %lld counted, %zu live", what, (long long)fx_device_bytes(c), live(DEVICE));
    size_t before = live(DEVICE), grown = 0;
    const int sizes[3] = {3, 5, 3}, bounds[3] = {n_bound_small, n_bound_large, n_bound_small};
    for (int step = 0; step < 3; step++) {
        Problem a(sizes[step], mode, bounds[step]), b(3, mode, bounds[step]);
        const FxProblem both[2] = {a.p, b.p};
        const int rc = fx_upload_batch(c, step == 1 ? 2 : 1, both);   // (the larger step has two agents as well)
        CHECK(rc == FX_OK, "%s: upload %d: %s", what, step, fx_last_error());
        CHECK((size_t)fx_device_bytes(c) == live(DEVICE), "%s: upload %d: %lld counted, %zu live", what, step, (long long)fx_device_bytes(c), live(DEVICE));
        if (step < 2) { CHECK(live(DEVICE) > before, "%s: upload %d did not grow (%zu)", what, step, live(DEVICE)); before = live(DEVICE); }
        if (step == 1) grown = live(DEVICE);
        if (step == 2) CHECK(live(DEVICE) == grown, "%s: the small step behind the large one changed %zu to %zu", what, grown, live(DEVICE));
    }
    CHECK(fx_destroy(c) == FX_OK, "%s: destroy", what);
    nothing_left(what);
}

int main() {
    // 1. create and destroy
    for (int agents : {1, 4}) {
        reset(0);
        FxContext *c = nullptr;
        CHECK(create(&c, agents) == FX_OK && c, "create(%d): %s", agents, fx_last_error());
        CHECK(live(STREAM) == 1 && live(EVENT) == 5 * 256, "create(%d): %zu streams, %zu events", agents, live(STREAM), live(EVENT));
        CHECK((size_t)fx_device_bytes(c) == live(DEVICE), "create(%d): %lld counted, %zu live", agents, (long long)fx_device_bytes(c), live(DEVICE));
        CHECK(fx_destroy(c) == FX_OK, "destroy");
        nothing_left("create and destroy");
    }
    // 2. every fallible call of a create, failing in turn
    reset(0);
    FxContext *c = nullptr;
    CHECK(create(&c, 4) == FX_OK, "create: %s", fx_last_error());
    const long n_calls = g_calls;
    fx_destroy(c);
    CHECK(n_calls > 5 * 256 + 20, "a create made only %ld fallible calls", n_calls);
    for (long k = 1; k <= n_calls; k++) {
        reset(k);
        c = reinterpret_cast<FxContext *>(&g_table);   // (anything but NULL)
        const int rc = create(&c, 4);
        CHECK(rc != FX_OK && c == nullptr, "create with call %ld failing: rc %d, *out %s", k, rc, c ? "not NULL" : "NULL");
        CHECK(live() == 0 && g_bad_frees == 0, "create with call %ld failing: %zu entries live, %d bad frees", k, live(), g_bad_frees);
        if (g_failed) break;
    }
    reset(n_calls + 1);   // (one past the last: nothing fails)
    CHECK(create(&c, 4) == FX_OK && c, "create with no call failing: %s", fx_last_error());
    fx_destroy(c);
    nothing_left("create behind the failing ones");
    // 3. the grow sites
    uploads("planes", FX_MODE_WRITE_BUNDLE, 1, 0, 0);
    uploads("boundary pair", FX_MODE_WRITE_BUNDLE | FX_MODE_ROAD_BOUNDARY, 0, 3, 5000);   // 64 KiB at first, then 2 x 160 KB
    uploads("obstacle scratch", FX_MODE_WRITE_BUNDLE, 2, 0, 0);
    reset(0);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok (%ld fallible calls per create)\n", n_calls);
    return 0;
}
