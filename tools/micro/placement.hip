// Where the hardware puts the waves of the split step's two big launches (tools/placement_census.py reads the records).
// Two stand-in kernels with the launch shape and the resource footprint of the real ones -- a probe store inside the real obstacle
// kernel moves its register count and with it its occupancy (profiles/r5/NOTES.md) --
//   walk      394 x 256 lanes, __launch_bounds__(256, 2), 164 VGPRs, the walk's dynamic LDS
//   obstacle  788 x 640 lanes, __launch_bounds__(1024, 1), 74 VGPRs, the obstacle kernel's dynamic LDS; workgroups >= 503 return at once
// each running a fixed chain of dependent FP64 FMAs.  Every wave records its hardware ids (HW_ID and XCC_ID registers), its start and
// end on the 100 MHz wall clock, its workgroup and wave index.
// The obstacle stand-in can give every chunk of the horizon its own chain length and map wave -> chunk through a 40-bit constant
// shifted by the wave index (four bits per wave), to measure what placing chunks by weight could gain on the measured placement.
// usage: placement [walk_lds obst_lds walk_iters obst_iters reps [w0,..,w9 [perm_hex [obst_waves]]]]
//        (one CSV line per wave on stdout, '#' lines are comments; w0..w9: chain length x 8 of chunks 0..9, default obst_iters each;
//        perm_hex: wave w runs chunk (perm >> 4 w) & 15, default 9876543210; obst_waves: 10 .. 16 waves per obstacle workgroup, the
//        waves past the tenth only wait at the barrier)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

struct WaveRec {
    unsigned hw_id, xcc_id, wg, wave;
    unsigned long long t0, t1;
};

#define GETREG(id, off, width) __builtin_amdgcn_s_getreg((id) | ((off) << 6) | (((width) - 1) << 11))
#define HW_REG_HW_ID 4
#define HW_REG_XCC_ID 20

__device__ __forceinline__ double fma_chain(double a, int iters) {
    const double b = 1.0000001, c = 1e-9;
    for (int i = 0; i < iters; i++) {
        a = fma(a, b, c); a = fma(a, b, c); a = fma(a, b, c); a = fma(a, b, c);
        a = fma(a, b, c); a = fma(a, b, c); a = fma(a, b, c); a = fma(a, b, c);
    }
    return a;
}

__device__ __forceinline__ void wave_record(WaveRec *out, int waves_per_wg, unsigned long long t0, unsigned hw, unsigned xcc) {
    const unsigned long long t1 = wall_clock64();
    if ((threadIdx.x & 63) == 0) {
        const unsigned wave = threadIdx.x >> 6;
        WaveRec r{hw, xcc, blockIdx.x, wave, t0, t1};
        out[(size_t)blockIdx.x * waves_per_wg + wave] = r;
    }
}

extern __shared__ double lds_dyn[];

__global__ __launch_bounds__(256, 2) void walk_standin(WaveRec *out, double *sink, int iters) {
    const unsigned long long t0 = wall_clock64();
    const unsigned hw = GETREG(HW_REG_HW_ID, 0, 32), xcc = GETREG(HW_REG_XCC_ID, 0, 4);
    asm volatile("" ::: "v163");   // the walk's 164 registers: three waves per SIMD
    lds_dyn[threadIdx.x] = (double)threadIdx.x;
    __syncthreads();
    const double a = fma_chain(lds_dyn[threadIdx.x ^ 1] * 1e-3, iters);
    sink[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = a;
    wave_record(out, 4, t0, hw, xcc);
}

struct ChunkIters { int n[10]; };

__global__ __launch_bounds__(1024, 1) void obstacle_standin(WaveRec *out, double *sink, ChunkIters tab, unsigned long long perm, int live) {
    if ((int)blockIdx.x >= live) return;
    // a launch with more than ten waves per workgroup (what a batch with a longer horizon beside this agent would ask for): the waves
    // without a chunk only meet the others at the workgroup's barrier, as in the real kernel
    if (threadIdx.x >= 640) {
        __syncthreads();
        __syncthreads();
        return;
    }
    const int chunk = (int)((perm >> (4 * __builtin_amdgcn_readfirstlane(threadIdx.x >> 6))) & 15ULL);
    const int iters = chunk == 0 ? tab.n[0] : chunk == 1 ? tab.n[1] : chunk == 2 ? tab.n[2] : chunk == 3 ? tab.n[3] : chunk == 4 ? tab.n[4] :
                      chunk == 5 ? tab.n[5] : chunk == 6 ? tab.n[6] : chunk == 7 ? tab.n[7] : chunk == 8 ? tab.n[8] : tab.n[9];
    const unsigned long long t0 = wall_clock64();
    const unsigned hw = GETREG(HW_REG_HW_ID, 0, 32), xcc = GETREG(HW_REG_XCC_ID, 0, 4);
    asm volatile("" ::: "v73");    // the obstacle kernel's 74 registers: six waves per SIMD
    lds_dyn[threadIdx.x] = (double)threadIdx.x;
    __syncthreads();
    const double a = fma_chain(lds_dyn[threadIdx.x ^ 1] * 1e-3, iters);
    sink[(size_t)blockIdx.x * 640 + threadIdx.x] = a;   // (threadIdx.x < 640 here)
    wave_record(out, 10, t0, hw, xcc);
    __syncthreads();
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static void dump(const char *name, const std::vector<WaveRec> &h, std::vector<float> all_us) {
    const float us = all_us.back();
    std::sort(all_us.begin(), all_us.end());
    printf("# times %s min_us %.2f median_us %.2f\n", name, all_us.front(), all_us[all_us.size() / 2]);
    unsigned long long tmin = ~0ULL;
    for (const WaveRec &r : h) if (r.wg != 0xffffffffu && r.t0 < tmin) tmin = r.t0;
    printf("# kernel %s event_us %.2f\n", name, us);
    for (const WaveRec &r : h) {
        if (r.wg == 0xffffffffu) continue;   // a workgroup that returned at once
        // HW_ID (gfx9): wave slot [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]; times in ns from the first wave's start
        printf("%s,%u,%u,%u,%u,%u,%u,%u,%u,%llu,%llu\n", name, r.wg, r.wave, r.xcc_id & 15u, (r.hw_id >> 13) & 7u, (r.hw_id >> 12) & 1u,
               (r.hw_id >> 8) & 15u, (r.hw_id >> 4) & 3u, r.hw_id & 15u, (r.t0 - tmin) * 10ULL, (r.t1 - tmin) * 10ULL);
    }
}

int main(int argc, char **argv) {
    const size_t walk_lds = argc > 1 ? (size_t)atol(argv[1]) : 39936, obst_lds = argc > 2 ? (size_t)atol(argv[2]) : 34000;
    const int walk_iters = argc > 3 ? atoi(argv[3]) : 800, obst_iters = argc > 4 ? atoi(argv[4]) : 200, reps = argc > 5 ? atoi(argv[5]) : 5;
    const int WALK_WGS = 394, OBST_WGS = 788, OBST_LIVE = 503;
    if (walk_lds < 256 * 8 || walk_lds > 64 * 1024 || obst_lds < 640 * 8 || obst_lds > 64 * 1024 || walk_iters < 1 || walk_iters > 100000 ||
        obst_iters < 1 || obst_iters > 100000 || reps < 1 || reps > 100) {
        fprintf(stderr, "arguments out of range\n");
        return 2;
    }
    ChunkIters tab;
    for (int q = 0; q < 10; q++) tab.n[q] = obst_iters;
    if (argc > 6 && sscanf(argv[6], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", &tab.n[0], &tab.n[1], &tab.n[2], &tab.n[3], &tab.n[4], &tab.n[5], &tab.n[6],
                           &tab.n[7], &tab.n[8], &tab.n[9]) != 10) {
        fprintf(stderr, "ten chain lengths expected\n");
        return 2;
    }
    const unsigned long long perm = argc > 7 ? strtoull(argv[7], nullptr, 16) : 0x9876543210ULL;
    unsigned seen = 0;
    for (int w = 0; w < 10; w++) {
        const unsigned q = (unsigned)((perm >> (4 * w)) & 15ULL);
        if (q > 9 || tab.n[w] < 1 || tab.n[w] > 100000) { fprintf(stderr, "arguments out of range\n"); return 2; }
        seen |= 1u << q;
    }
    if (seen != 0x3ffu) { fprintf(stderr, "perm is no permutation of the ten chunks\n"); return 2; }
    const int obst_waves = argc > 8 ? atoi(argv[8]) : 10;   // waves per workgroup of the obstacle launch (the first ten have a chunk)
    if (obst_waves < 10 || obst_waves > 16) { fprintf(stderr, "10 .. 16 waves per workgroup\n"); return 2; }
    const size_t n_walk = (size_t)WALK_WGS * 4, n_obst = (size_t)OBST_WGS * 10;
    WaveRec *d_rec;
    double *d_sink;
    CHECK(hipMalloc(&d_rec, sizeof(WaveRec) * n_obst));            // (n_obst > n_walk)
    CHECK(hipMalloc(&d_sink, sizeof(double) * OBST_WGS * 640));    // (788 x 640 > 394 x 256)
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("# device %s CUs %d\n# columns kernel,wg,wave,xcc,se,sh,cu,simd,slot,t0_ns,t1_ns\n", prop.name, prop.multiProcessorCount);
    printf("# walk_lds %zu obst_lds %zu walk_iters %d obst_iters %d reps %d (the last repetition is recorded)\n", walk_lds, obst_lds, walk_iters,
           obst_iters, reps);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<WaveRec> h(n_obst);
    float ms = 0;
    std::vector<float> us;
    for (int r = 0; r < reps; r++) {
        CHECK(hipMemset(d_rec, 0xff, sizeof(WaveRec) * n_obst));
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(walk_standin, dim3(WALK_WGS), dim3(256), walk_lds, 0, d_rec, d_sink, walk_iters);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        us.push_back(ms * 1e3f);
    }
    CHECK(hipMemcpy(h.data(), d_rec, sizeof(WaveRec) * n_walk, hipMemcpyDeviceToHost));
    dump("walk", std::vector<WaveRec>(h.begin(), h.begin() + n_walk), us);
    us.clear();
    for (int r = 0; r < reps; r++) {
        CHECK(hipMemset(d_rec, 0xff, sizeof(WaveRec) * n_obst));
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(obstacle_standin, dim3(OBST_WGS), dim3(64 * obst_waves), obst_lds, 0, d_rec, d_sink, tab, perm, OBST_LIVE);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        us.push_back(ms * 1e3f);
    }
    CHECK(hipMemcpy(h.data(), d_rec, sizeof(WaveRec) * n_obst, hipMemcpyDeviceToHost));
    printf("# obstacle chain lengths %d,%d,%d,%d,%d,%d,%d,%d,%d,%d perm %llx waves per workgroup %d\n", tab.n[0], tab.n[1], tab.n[2], tab.n[3], tab.n[4], tab.n[5], tab.n[6],
           tab.n[7], tab.n[8], tab.n[9], perm, obst_waves);
    dump("obstacle", h, us);
    return 0;
}
