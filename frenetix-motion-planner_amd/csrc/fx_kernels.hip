// fx_kernels.hip -- the one translation unit of libfxplan.so with device code: it includes every kernel family (fx_*_kernel.h,
// fx_select.h) and holds their launchers (declared in fx_launch.h, called by fx_api*.hip) and a few kernels too small for a header
// of their own.  What runs when is decided by the callers (fx_policy.h); the evaluation pipeline is described in fx_eval_kernel.h.
#include <hip/hip_ext.h>

#include <atomic>

#include "fx_eval_kernel.h"
#include "fx_eval_grid_kernel.h"
#include "fx_eval_list_kernel.h"
#include "fx_obstacle_kernel.h"
#include "fx_step_kernel.h"
#include "fx_risk_kernel.h"
#include "fx_predprob_kernel.h"
#include "fx_gather_kernel.h"
#include "fx_sort_kernel.h"
#include "fx_selftest_kernel.h"
#include "fx_launch.h"   // every launcher below is held to its declaration
#include "fx_pass.h"

using fxk::wave_count;

// the vector unit's row_bcast data-parallel controls (fx_walk.h wave_max_u32, wave_min_u64 below) exist on the GFX9 family only
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "libfxplan's kernels are written for gfx950 (row_bcast DPP controls, wave64): build with --offload-arch=gfx950"
#endif

// slot of the calling thread's current device in the per-device tables of the launchers
#define FX_MAX_DEVICES 64
static inline int fx_device_slot() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
    return d % FX_MAX_DEVICES;
}

// Let `Kernel` be launched with lds_bytes of dynamic LDS: above 48 KiB the limit has to be raised, PER DEVICE (the attribute is per
// device; the call costs microseconds: once per size, not per launch).  The table holds the largest size each device has been
// enabled for -- one table per kernel specialisation; relaxed atomics: two threads at worst both set the attribute.  set_to: the
// size to enable instead of lds_bytes (a kernel whose largest size is known).
template <auto Kernel>
static hipError_t fx_allow_dynamic_lds(size_t lds_bytes, size_t set_to = 0) {
    static std::atomic<size_t> lds_set_[FX_MAX_DEVICES];
    std::atomic<size_t> &hw_ = lds_set_[fx_device_slot()];
    if (lds_bytes > 48 * 1024 && lds_bytes > hw_.load(std::memory_order_relaxed)) {
        const size_t bytes = set_to ? set_to : lds_bytes;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        hw_.store(bytes, std::memory_order_relaxed);
    }
    return hipSuccess;
}

#ifdef FX_CULL_STATS
__device__ unsigned long long fx_cull_stats[16];
__device__ double fx_probe_bound = 1e300;
extern "C" int fx_probe_bound_set(double v) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(fx_probe_bound), &v, sizeof(v), 0, hipMemcpyHostToDevice); }
extern "C" int fx_cull_stats_read(unsigned long long *out, int reset) {
    int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fx_cull_stats), sizeof(fx_cull_stats), 0, hipMemcpyDeviceToHost);
    if (reset) {
        unsigned long long z[16] = {0};
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(fx_cull_stats), z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return rc;
}
#endif
#ifdef FX_PROBE
__device__ unsigned long long fx_probe_stamps[FX_PROBE_WAVES * FX_PROBE_SLOTS];
extern "C" int fx_probe_read(unsigned long long *out, size_t n_words) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fx_probe_stamps), n_words * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
__device__ unsigned long long fx_probe_stamps_obs[FX_PROBE_WAVES * FX_PROBE_SLOTS];
extern "C" int fx_probe_read_obs(unsigned long long *out, size_t n_words) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fx_probe_stamps_obs), n_words * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

// (fx_package_gather: fx_tail.h)
__global__ __launch_bounds__(256) void fx_package_kernel(const DevProblem *__restrict__ probs, const double *__restrict__ winner,
                                                         double *host_pkg, int stride, int plane_rows, unsigned long long seq) {
    double *out = host_pkg + (size_t)blockIdx.x * stride;
    fxk::fx_package_gather<false>(probs[blockIdx.x], reinterpret_cast<const long long *>(winner)[2 * blockIdx.x + 1], out, plane_rows,
                                  (int)threadIdx.x, 256);
    __syncthreads();   // (every wave's package words are acknowledged: fx_tail.h, st_host / drain_stores)
    if (threadIdx.x == 0) fxk::st_host(reinterpret_cast<unsigned long long *>(out + stride - 1), seq);
}

extern "C" hipError_t fx_launch_package(const DevProblem *d_probs, int n_agents, const double *winner, double *host_pkg, int stride,
                                        int plane_rows, unsigned long long seq, hipStream_t stream) {
    hipLaunchKernelGGL(fx_package_kernel, dim3(n_agents), dim3(256), 0, stream, d_probs, winner, host_pkg, stride, plane_rows, seq);
    return hipGetLastError();
}

#include "fx_select.h"   // fx_select_kernel

// top-k: slices per agent, entries per lane of the one-wave kernels -- the sizes at which fx_launch_topk changes kernels
#define FX_TOPK_SLICES 64
#define FX_TOPK_R 32
#include "fx_topk_kernel.h"   // fx_topk_*_kernel
#include "fx_rescore_kernel.h"   // fxrs::fx_rescore_*_kernel
#include "fx_rescore_batch_kernel.h"   // fxrs::fx_rescore_batch_*_kernel
#include "fx_hypotheses_kernel.h"   // fxhy::fx_hyp_*_kernel
#include "fx_hypotheses_batch_kernel.h"   // fxhy::fx_hyp_batch_*_kernel

// Copy a small device buffer (the all-gathered survivors) into pinned host memory and publish a sequence word:
// the host polls instead of paying for a D2H copy + stream synchronisation.
__global__ __launch_bounds__(256) void fx_publish_kernel(const double *__restrict__ src, int n, double *host_dst,
                                                         unsigned long long *host_seq, unsigned long long seq) {
    for (int i = threadIdx.x; i < n; i += 256) fxk::put_host(host_dst + i, src[i]);
    fxk::drain_stores();  // per wave: its stores are acknowledged before the barrier lets thread 0 send the sequence word
    __syncthreads();
    if (threadIdx.x == 0) fxk::st_host(host_seq, seq);
}

extern "C" hipError_t fx_launch_publish(const double *src, int n, double *host_dst, unsigned long long *host_seq,
                                        unsigned long long seq, hipStream_t stream) {
    hipLaunchKernelGGL(fx_publish_kernel, dim3(1), dim3(256), 0, stream, src, n, host_dst, host_seq, seq);
    return hipGetLastError();
}

// Staging copy of a plan step's rewritten inputs: the kernel reads the pinned (mapped) staging block over the bus and writes
// the device copy, 16 B per lane.  For the 1 - 150 KB a state update touches this lands in a few microseconds behind the
// launch, where a DMA-engine copy of the same bytes costs its submission latency first (measured: tools/upload_step.py).
__global__ __launch_bounds__(256) void fx_stage_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int n16) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}

extern "C" hipError_t fx_launch_stage(const void *src_mapped, void *dst, size_t bytes, hipStream_t stream) {
    const int n16 = (int)(bytes / 16);
    const int blocks = std::min(256, std::max(1, (n16 + 255) / 256));
    hipLaunchKernelGGL(fx_stage_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(src_mapped),
                       reinterpret_cast<uint4 *>(dst), n16);
    return hipGetLastError();
}

// element-wise check of the fx_math kernels (tests/test_hip_math.py)
// probe of the host-write path (fx_api.hip, probe_host_writes): every workgroup -- they are spread over all XCDs -- copies the same
// 64 bytes of the arena into its own slot, so that a stale copy of the line in ANY XCD's L2 shows
__global__ void fx_probe_read_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst) {
    if (threadIdx.x < 4) dst[blockIdx.x * 4 + threadIdx.x] = src[threadIdx.x];
}
extern "C" hipError_t fx_launch_probe_read(const void *src, void *dst, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL(fx_probe_read_kernel, dim3(blocks), dim3(64), 0, stream, reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(dst));
    return hipGetLastError();
}

__global__ void fx_math_test_kernel(int n, const double *__restrict__ x, double *__restrict__ at, double *__restrict__ sn,
                                    double *__restrict__ cs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    at[i] = fxm::atan(x[i]);
    fxm::sincos(x[i], &sn[i], &cs[i]);
}

extern "C" hipError_t fx_launch_math_test(int n, const double *x, double *at, double *sn, double *cs, hipStream_t stream) {
    hipLaunchKernelGGL(fx_math_test_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, x, at, sn, cs);
    return hipGetLastError();
}

// one primitive of the kernels' arithmetic, elementwise (fx_selftest_kernel.h; tests/test_device_math.py)
extern "C" hipError_t fx_launch_selftest(int op, int n, const SelftestArgs *args, hipStream_t stream) {
    if (n < 1 || n > FX_SELFTEST_MAX_N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fx_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, op, n, *args);
    return hipGetLastError();
}

// ---- launchers (called from fx_api.hip) ----
// Launch the evaluation kernel specialised for (G lanes per candidate, bundle, obstacles, extra costs, occupancy target).
extern "C" hipError_t fx_launch_eval(const DevProblem *d_probs, int n_agents, int max_blocks, size_t lds_bytes, int G,
                                     bool bundle, bool obst, bool extra, int wpe, hipEvent_t ev_start, hipEvent_t ev_stop,
                                     FuseArgs fuse, hipStream_t stream) {
    dim3 grid(max_blocks, n_agents), block(FX_BLOCK);
#define FX_LAUNCH(Gv, B, O, E, W)                                                                                \
    do {                                                                                                        \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fx_eval_kernel<Gv, B, O, E, W>>(lds_bytes); e_ != hipSuccess) return e_; \
        hipExtLaunchKernelGGL((fx_eval_kernel<Gv, B, O, E, W>), grid, block, lds_bytes, stream, ev_start, ev_stop, 0, d_probs, fuse); \
        return hipGetLastError();                                                                               \
    } while (0)
#define FX_BO(Gv, W)                                                          \
    do {                                                                      \
        if (bundle && obst) FX_LAUNCH(Gv, true, true, false, W);              \
        if (bundle) FX_LAUNCH(Gv, true, false, false, W);                     \
        if (obst) FX_LAUNCH(Gv, false, true, false, W);                       \
        FX_LAUNCH(Gv, false, false, false, W);                                \
    } while (0)
    // four waves per SIMD (128 VGPRs) only exists for the plain select-only walk: with the bundle stores or the obstacle
    // stage that budget spills hundreds of bytes per lane to scratch -- slower than three waves, and kernels with that much
    // private memory faulted on this platform when a process used a second stream
#define FX_W(Gv)                                                          \
    do {                                                                  \
        if (wpe >= 4 && !bundle && !obst) FX_LAUNCH(Gv, false, false, false, 4); \
        if (wpe >= 3) FX_BO(Gv, 3);                                       \
        FX_BO(Gv, 2);                                                     \
    } while (0)
    if (extra) {  // windowed costs: one lane per candidate
        if (bundle && obst) FX_LAUNCH(1, true, true, true, 2);
        if (bundle) FX_LAUNCH(1, true, false, true, 2);
        if (obst) FX_LAUNCH(1, false, true, true, 2);
        FX_LAUNCH(1, false, false, true, 2);
    }
    switch (G) {
    case 32: FX_BO(32, 1);   // planner-sized sampling matrices: one or two steps per lane; one wave per SIMD is all they fill, so the
                             // allocator may use the whole register file (at two waves per SIMD: 12 registers spilled to scratch)
    case 16: FX_BO(16, 2);
    case 8: FX_W(8);
    case 4: FX_W(4);
    case 2: FX_W(2);
    default: FX_W(1);
    }
#undef FX_W
#undef FX_BO
#undef FX_LAUNCH
}

// Grid (t x v x d) specialisation with the shared longitudinal table; lds_bytes includes the rows.
extern "C" hipError_t fx_launch_eval_grid(const DevProblem *d_probs, int n_agents, int max_blocks, int block_size,
                                          size_t lds_bytes, int G, bool bundle, bool obst, int wpe, bool wsplit,
                                          hipEvent_t ev_start, hipEvent_t ev_stop, FuseArgs fuse, hipStream_t stream) {
    dim3 grid(max_blocks, n_agents), block(block_size);
#define FX_LAUNCH(Gv, B, O, W, WS)                                                                                 \
    do {                                                                                                          \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fx_eval_grid_kernel<Gv, B, O, W, WS>>(lds_bytes); e_ != hipSuccess) return e_; \
        hipExtLaunchKernelGGL((fx_eval_grid_kernel<Gv, B, O, W, WS>), grid, block, lds_bytes, stream, ev_start, ev_stop, 0, d_probs, fuse); \
        return hipGetLastError();                                                                                 \
    } while (0)
#define FX_BO(Gv, W, WS)                                           \
    do {                                                           \
        if (bundle && obst) FX_LAUNCH(Gv, true, true, W, WS);      \
        if (bundle) FX_LAUNCH(Gv, true, false, W, WS);             \
        if (obst) FX_LAUNCH(Gv, false, true, W, WS);               \
        FX_LAUNCH(Gv, false, false, W, WS);                        \
    } while (0)
#define FX_W(Gv, WS)                                                          \
    do {                                                                      \
        if (wpe >= 4 && !bundle && !obst) FX_LAUNCH(Gv, false, false, 4, WS); \
        if (wpe >= 3) FX_BO(Gv, 3, WS);                                       \
        FX_BO(Gv, 2, WS);                                                     \
    } while (0)
    if (wsplit && G > 1) {
        switch (G) {
        case 4: FX_W(4, true);
        default: FX_W(2, true);
        }
    }
    switch (G) {
    case 32: FX_BO(32, 2, false);   // planner-sized grids: one or two steps per lane, one occupancy target
    case 16: FX_BO(16, 2, false);
    case 8: FX_W(8, false);
    case 4: FX_W(4, false);
    case 2: FX_W(2, false);
    default: FX_W(1, false);
    }
#undef FX_W
#undef FX_BO
#undef FX_LAUNCH
}

// The obstacle stage as its own kernel (fx_obstacle_kernel.h): grid = (max tiles x chunks, n_agents), one wave per item,
// dynamic LDS = CH * K * 48 B.
extern "C" hipError_t fx_launch_obstacle(const DevProblem *d_probs, int n_agents, int max_items, size_t lds_bytes, int CH,
                                         hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream, int wg_waves, int max_tiles,
                                         const DevProblem *head) {
    // wg_waves > 0: one workgroup of wg_waves waves per tile (the chunks meet in LDS), grid = (max_tiles, n_agents)
    // head (one agent): the HEAD kernels, with the step header in their leading arguments (fx_obstacle_kernel.h, ObstHead)
    const bool hd = head && n_agents == 1;
    const DevProblem none{};
    const DevProblem &h = hd ? *head : none;
#define FX_LAUNCH_K(CHv, WGv, HDv, grid, block)                                                                                         \
    do {                                                                                                                            \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fxk::fx_obstacle_kernel<CHv, 4, WGv, HDv>>(lds_bytes); e_ != hipSuccess) return e_; \
        hipExtLaunchKernelGGL((fxk::fx_obstacle_kernel<CHv, 4, WGv, HDv>), grid, block, lds_bytes, stream, ev_start, ev_stop, 0, d_probs,   \
                              h.obs_list, h.counters, h.obs_hot, h.C, h.S, h.K, h.mode);                                             \
        return hipGetLastError();                                                                                                   \
    } while (0)
#define FX_LAUNCH(CHv)                                                                                                                \
    do {                                                                                                                            \
        if (wg_waves > 0) {                                                                                                         \
            if (hd) FX_LAUNCH_K(CHv, true, true, dim3(max_tiles, n_agents), dim3(64 * wg_waves));                                     \
            FX_LAUNCH_K(CHv, true, false, dim3(max_tiles, n_agents), dim3(64 * wg_waves));                                            \
        }                                                                                                                           \
        if (hd) FX_LAUNCH_K(CHv, false, true, dim3(max_items, n_agents), dim3(64));                                                   \
        FX_LAUNCH_K(CHv, false, false, dim3(max_items, n_agents), dim3(64));                                                          \
    } while (0)
    if (CH == 2) FX_LAUNCH(2);
    if (CH == 3) FX_LAUNCH(3);
    if (CH == 5) FX_LAUNCH(5);
#undef FX_LAUNCH
#undef FX_LAUNCH_K
    return hipErrorInvalidValue;
}

// The whole step in one launch (fx_step_kernel.h): grid = (blocks, n_agents), 256 lanes.  fx_step_kernel_capacity: how many of
// its workgroups the device holds at once with `lds_bytes` of dynamic LDS (the grid barrier needs them all resident).
#define FX_STEP_CASES(X) X(3) X(5) X(8)
extern "C" hipError_t fx_step_kernel_capacity(int CH, size_t lds_bytes, int *blocks_out) {
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
#define FX_CAP(CHv)                                                                                                              \
    if (CH == CHv) {                                                                                                             \
        if (lds_bytes > 48 * 1024) {                                                                                             \
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fx_step_kernel<CHv>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)lds_bytes);                                                                             \
            if (e != hipSuccess) return e;                                                                                       \
        }                                                                                                                        \
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fx_step_kernel<CHv>, FX_BLOCK, lds_bytes);                     \
        if (e != hipSuccess) return e;                                                                                           \
        *blocks_out = per_cu * cus;                                                                                              \
        return hipSuccess;                                                                                                       \
    }
    FX_STEP_CASES(FX_CAP)
#undef FX_CAP
    return hipErrorInvalidValue;
}
extern "C" hipError_t fx_launch_step(const DevProblem *d_probs, int n_agents, int blocks, size_t lds_bytes, int CH, hipEvent_t ev_start,
                                     hipEvent_t ev_stop, FuseArgs fuse, StepArgs sa, hipStream_t stream) {
#define FX_LAUNCH(CHv)                                                                                                           \
    if (CH == CHv) {                                                                                                             \
        hipExtLaunchKernelGGL((fx_step_kernel<CHv>), dim3(blocks, n_agents), dim3(FX_BLOCK), lds_bytes, stream, ev_start, ev_stop, 0, \
                              d_probs, fuse, sa);                                                                                \
        return hipGetLastError();                                                                                                \
    }
    FX_STEP_CASES(FX_LAUNCH)
#undef FX_LAUNCH
    return hipErrorInvalidValue;
}

// head (as in fx_launch_obstacle): the host's copy of the ONE agent's problem, whose fields the kernel's first loads need travel
// as leading kernel arguments (fx_select.h, SelectHead); nullptr for a batch.
extern "C" hipError_t fx_launch_select(const DevProblem *d_probs, int n_agents, int64_t max_candidates, unsigned long long *host_result,
                                       unsigned long long seq, double *dev_winner, double *host_pkg, int pkg_stride, int pkg_plane_rows,
                                       hipStream_t stream, const DevProblem *head) {
    // one slice per ~4 096 candidates of the largest agent, at least 32 (the small-step tuning), a power of two, at most 512
    int slices = FX_SELECT_SLICES_MIN;
    while (slices < FX_SELECT_SLICES_MAX && (int64_t)slices * 4096 < max_candidates) slices *= 2;
    // batched launches: keep the grid around a thousand workgroups (every workgroup reduces all of an agent's partials)
    while (slices > FX_SELECT_SLICES_MIN && (int64_t)slices * n_agents > 2048) slices /= 2;
    const DevProblem none{};   // (the header's counts are 32-bit: a larger agent reads its problem like a batch)
    const DevProblem &h = head && n_agents == 1 && head->C < ((int64_t)1 << 31) ? *head : none;
    hipLaunchKernelGGL(fx_select_kernel, dim3(slices, n_agents), dim3(256), 0, stream, d_probs, h.flags, h.cost, h.part_cost, h.part_idx,
                       (int32_t)h.C, (int32_t)((h.C + slices - 1) / slices), h.n_blocks, h.mode, h.counters, host_result, seq, dev_winner,
                       host_pkg, pkg_stride, pkg_plane_rows);
    return hipGetLastError();
}

extern "C" hipError_t fx_launch_topk(const DevProblem *d_probs, int n_agents, int64_t max_candidates, int k, double *scr_cost,
                                     long long *scr_idx, double *out_cost, long long *out_idx, hipStream_t stream) {
    // one wave per slice / per agent where the entries fit its registers (fx_topk_*_wave_kernel), the general kernels beyond
    const int64_t per = (max_candidates + FX_TOPK_SLICES - 1) / FX_TOPK_SLICES;
    if (per <= 64 * FX_TOPK_R)
        hipLaunchKernelGGL(fx_topk_slice_wave_kernel, dim3(FX_TOPK_SLICES, n_agents), dim3(64), 0, stream, d_probs, k, scr_cost, scr_idx);
    else
        hipLaunchKernelGGL(fx_topk_slice_kernel, dim3(FX_TOPK_SLICES, n_agents), dim3(256), 0, stream, d_probs, k, scr_cost, scr_idx);
    if (FX_TOPK_SLICES * k <= 64 * FX_TOPK_R)
        hipLaunchKernelGGL(fx_topk_merge_wave_kernel, dim3(n_agents), dim3(64), 0, stream, k, scr_cost, scr_idx, out_cost, out_idx);
    else
        hipLaunchKernelGGL(fx_topk_merge_kernel, dim3(n_agents), dim3(256), 0, stream, k, scr_cost, scr_idx, out_cost, out_idx);
    return hipGetLastError();
}

// trajectory risk (fx_risk_kernel.h; DESIGN.md sections 11, 13 and 17) over the w.n listed candidates: the walk in batches of
// it.nb candidates -- per batch the (tile, chunk, obstacle) items and the finish kernel; the plain one, or with col / out_occ the
// detail one -- and the arg-min of ego + obst into out_idx[0]; then, cost != null, the cost pass over the columns and the arg-min of
// its total into out_idx[1]; then, resp != null, the re-sum of the step's cost with the responsibility term and its arg-min into
// resp_idx[0 .. 1].  ev_start / ev_stop (may be null) bracket all of them.
extern "C" hipError_t fx_launch_risk(const RiskWalkArgs *walk, const RiskItemArgs *items, double *out_ego, double *out_obst, double *col,
                                     double *out_occ, const RiskCostArgs *cost, long long *out_idx, hipEvent_t ev_start,
                                     hipEvent_t ev_stop, hipStream_t stream, const RespSumArgs *resp, long long *resp_idx) {
    const RiskWalkArgs &w = *walk;
    const RiskItemArgs &it = *items;
    if (ev_start) { hipError_t e = hipEventRecord(ev_start, stream); if (e != hipSuccess) return e; }
    const dim3 grid((unsigned)((w.n + 255) / 256));
    for (int64_t j0 = 0; j0 < w.n; j0 += it.nb) {
        const int64_t m = std::min<int64_t>(it.nb, w.n - j0);
        const dim3 igrid((unsigned)((m + 63) / 64), (unsigned)it.chunks, (unsigned)w.K), fgrid((unsigned)((m + 255) / 256));
        if (col) {
            if (w.K > 0 && w.S > 1) hipLaunchKernelGGL(fxrisk::fx_risk_item_kernel<true>, igrid, dim3(64), 0, stream, w, it, j0);
            hipLaunchKernelGGL(fxrisk::fx_risk_items_finish_kernel<true>, fgrid, dim3(256), 0, stream, w, it, j0, out_ego, out_obst, col, out_occ);
        } else {
            if (w.K > 0 && w.S > 1) hipLaunchKernelGGL(fxrisk::fx_risk_item_kernel<false>, igrid, dim3(64), 0, stream, w, it, j0);
            hipLaunchKernelGGL(fxrisk::fx_risk_items_finish_kernel<false>, fgrid, dim3(256), 0, stream, w, it, j0, out_ego, out_obst, col, out_occ);
        }
    }
    hipLaunchKernelGGL(fxrisk::fx_risk_argmin_kernel, dim3(1), dim3(1024), 0, stream, out_ego, out_obst, w.n, w.ids, out_idx);
    if (cost) {
        if (w.n > 0) hipLaunchKernelGGL(fxrisk::fx_risk_cost_kernel, grid, dim3(256), 0, stream, *cost);
        hipLaunchKernelGGL(fxrisk::fx_risk_cost_argmin_kernel, dim3(1), dim3(1024), 0, stream, cost->out + 5 * (size_t)w.n, w.n, w.ids,
                           out_idx + 1);
    }
    if (resp) {
        if (w.n > 0) hipLaunchKernelGGL(fxrisk::fx_resp_finish_kernel, grid, dim3(256), 0, stream, *resp);
        hipLaunchKernelGGL(fxpp::fx_predprob_argmin_kernel, dim3(1), dim3(1024), 0, stream, resp->total, w.n, w.ids, w.flags, resp_idx);
    }
    if (ev_stop) { hipError_t e = hipEventRecord(ev_stop, stream); if (e != hipSuccess) return e; }
    return hipGetLastError();
}

// collision probability as the prediction cost (fx_predprob_kernel.h) over the a.n listed candidates, in
// batches of a.nb: per batch the (tile, chunk, obstacle) items and the finish kernel, then the arg-min of the total into out_idx.
// Steps per chunk: fx_predprob_chunk_steps (fx_api_risk.hip).  ev_start / ev_stop bracket all launches.
extern "C" hipError_t fx_launch_predprob(const PredProbArgs *args, long long *out_idx, hipEvent_t ev_start, hipEvent_t ev_stop,
                                         hipStream_t stream) {
    const PredProbArgs &a = *args;
    hipError_t e;
    if (ev_start && (e = hipEventRecord(ev_start, stream)) != hipSuccess) return e;
    const int cs = fx_predprob_chunk_steps(a.n, a.S, a.K);
    const unsigned chunks = (unsigned)((std::max(a.S - 1, 1) + cs - 1) / cs);
    for (int64_t j0 = 0; j0 < a.n; j0 += a.nb) {
        const int64_t m = std::min<int64_t>(a.nb, a.n - j0);
        if (a.source == FX_PRED_SOURCE_PROBABILITY && a.K > 0 && a.S > 1)
            hipLaunchKernelGGL(fxpp::fx_predprob_item_kernel, dim3((unsigned)((m + 63) / 64), chunks, (unsigned)a.K), dim3(64), 0, stream, a, j0, cs);
        hipLaunchKernelGGL(fxpp::fx_predprob_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, a, j0);
    }
    hipLaunchKernelGGL(fxpp::fx_predprob_argmin_kernel, dim3(1), dim3(1024), 0, stream, a.total, a.n, a.ids, a.flags, out_idx);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_stop && (e = hipEventRecord(ev_stop, stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The launches of a pass over several agents in one call (DESIGN.md sections 18 to 21), the one sequence of the four launchers below:
// per round ONE item launch over the flat items of all its rows and ONE finish launch, then what `tail` launches once behind the
// last round.  t: the device tables; rounds: the host's account of them (fx_api_risk.hip builds both).  ev_start / ev_stop
// bracket all launches.
template <class Row, class ItemKernel, class FinishKernel, class Tail>
static hipError_t launch_rounds(const BatchTable<Row> &t, const FxItemRound *rounds, int n_rounds, ItemKernel item, FinishKernel finish,
                                hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream, Tail tail) {
    hipError_t e;
    if (ev_start && (e = hipEventRecord(ev_start, stream)) != hipSuccess) return e;
    for (int r = 0; r < n_rounds; r++) {
        const FxItemRound &q = rounds[r];
        if (q.items > 0) hipLaunchKernelGGL(item, dim3((unsigned)q.items), dim3(64), 0, stream, t.rows + q.row0, t.item0 + q.row0, q.n_rows);
        hipLaunchKernelGGL(finish, dim3((unsigned)q.fin_blocks), dim3(256), 0, stream, t.rows + q.row0, t.fin0 + q.row0, q.n_rows);
    }
    tail();
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_stop && (e = hipEventRecord(ev_stop, stream)) != hipSuccess) return e;
    return hipSuccess;
}

// the prediction-probability pass (section 18): behind the rounds one arg-min launch with a workgroup per agent -- 2 R + 1 launches
extern "C" hipError_t fx_launch_predprob_batch(const PredProbBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                               hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream) {
    return launch_rounds(*t, rounds, n_rounds, fxpp::fx_predprob_batch_item_kernel, fxpp::fx_predprob_batch_finish_kernel, ev_start, ev_stop,
                         stream, [&] {
        hipLaunchKernelGGL(fxpp::fx_predprob_batch_argmin_kernel, dim3((unsigned)t->n_agents), dim3(1024), 0, stream, t->rows, t->agent_row, out_idx);
    });
}

// the responsibility pass (fx_risk_kernel.h; section 19): behind the rounds the cost kernel, the re-sum and the arg-min once each
// over all listed agents -- 2 R + 3 launches
extern "C" hipError_t fx_launch_risk_batch(const RiskBatchArgs *a, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                           hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream) {
    return launch_rounds(a->t, rounds, n_rounds, fxrisk::fx_risk_batch_item_kernel, fxrisk::fx_risk_batch_finish_kernel, ev_start, ev_stop,
                         stream, [&] {
        const int32_t n = a->t.n_agents;
        if (a->blocks > 0) {
            hipLaunchKernelGGL(fxrisk::fx_risk_batch_cost_kernel, dim3((unsigned)a->blocks), dim3(256), 0, stream, a->cost, a->blk0, n);
            hipLaunchKernelGGL(fxrisk::fx_risk_batch_sum_kernel, dim3((unsigned)a->blocks), dim3(256), 0, stream, a->sum, a->blk0, n);
        }
        hipLaunchKernelGGL(fxrisk::fx_risk_batch_argmin_kernel, dim3((unsigned)n), dim3(1024), 0, stream, a->sum, out_idx);
    });
}

// the plain risk pass, each agent with an id list or none (section 20): behind the rounds one arg-min launch with a workgroup per
// agent -- 2 R + 1 launches
extern "C" hipError_t fx_launch_risk_list_batch(const RiskListBatchArgs *t, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                                hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream) {
    return launch_rounds(*t, rounds, n_rounds, fxrisk::fx_risk_list_batch_item_kernel, fxrisk::fx_risk_list_batch_finish_kernel, ev_start,
                         ev_stop, stream, [&] {
        hipLaunchKernelGGL(fxrisk::fx_risk_list_batch_argmin_kernel, dim3((unsigned)t->n_agents), dim3(1024), 0, stream, t->rows, t->agent_row,
                           out_idx);
    });
}

// the detail and cost passes, each agent with an id list or none and with cost parameters or none (section 21; the finish kernel
// is the responsibility pass's and the risk arg-min the plain pass's, as they stand): behind the rounds the risk arg-min with a
// workgroup per agent and, where an agent has cost parameters, the cost kernel and the cost arg-min once each over those agents,
// and, where the caller asked for a per-obstacle column, one launch that lays the agents' column blocks into the call's
// concatenated columns -- 2 R + 4 launches at most.  out_idx [n_agents] the risk arg-min, cost_idx [n_cost] the cost arg-min.
extern "C" hipError_t fx_launch_risk_costs_batch(const RiskCostBatchArgs *a, const FxItemRound *rounds, int n_rounds, long long *out_idx,
                                                 long long *cost_idx, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream) {
    return launch_rounds(a->t, rounds, n_rounds, fxrisk::fx_risk_costs_batch_item_kernel, fxrisk::fx_risk_batch_finish_kernel, ev_start,
                         ev_stop, stream, [&] {
        hipLaunchKernelGGL(fxrisk::fx_risk_list_batch_argmin_kernel, dim3((unsigned)a->t.n_agents), dim3(1024), 0, stream, a->t.rows,
                           a->t.agent_row, out_idx);
        if (a->n_cost > 0) {
            if (a->blocks > 0)
                hipLaunchKernelGGL(fxrisk::fx_risk_costs_batch_cost_kernel, dim3((unsigned)a->blocks), dim3(256), 0, stream, a->cost, a->blk0,
                                   a->n_cost);
            hipLaunchKernelGGL(fxrisk::fx_risk_costs_batch_argmin_kernel, dim3((unsigned)a->n_cost), dim3(1024), 0, stream, a->cost, cost_idx);
        }
        if (a->seg_blocks > 0)
            hipLaunchKernelGGL(fxrisk::fx_risk_costs_batch_gather_kernel, dim3((unsigned)a->seg_blocks), dim3(256), 0, stream, a->seg,
                               a->seg_blk0, a->n_seg);
    });
}

// batched candidate read-back (fx_gather_kernel.h): one workgroup per listed candidate
extern "C" hipError_t fx_launch_gather_candidates(const GatherArgs *args, const int64_t *d_ids, int64_t n, unsigned long long *d_out,
                                                  hipStream_t stream) {
    if (n > 0)
        hipLaunchKernelGGL(fx_gather_candidates_kernel, dim3((unsigned)n), dim3(FX_GATHER_BLOCK), 0, stream, *args, d_ids, n, d_out);
    return hipGetLastError();
}

// list form of the generic kernel (fx_eval_list_kernel.h): the n = clone.C listed candidates of ONE agent into its sparse block;
// d_prob is the clone of the agent's problem, lds_bytes as for fx_launch_eval.
// With d_rows: the rows form (fx_eval_list_rows_kernel) -- n_rows rows of one variant (lanes, obst, extra),
// n the longest of their lists and lds_bytes the largest of their needs; d_prob and d_ids are not read.  Either event may be null:
// a call's first launch takes the start event and its last one the stop event.
template <int G, bool O, bool E>
static hipError_t fx_launch_eval_list_rows(const EvalListRow *d_rows, int n_rows, int64_t n, size_t lds_bytes, hipEvent_t ev_start,
                                           hipEvent_t ev_stop, hipStream_t stream) {
    if (const hipError_t e = fx_allow_dynamic_lds<&fx_eval_list_rows_kernel<G, O, E>>(lds_bytes); e != hipSuccess) return e;
    constexpr int CPB = FX_BLOCK / G;
    hipExtLaunchKernelGGL((fx_eval_list_rows_kernel<G, O, E>), dim3((unsigned)((n + CPB - 1) / CPB), (unsigned)n_rows), dim3(FX_BLOCK), lds_bytes,
                          stream, ev_start, ev_stop, 0, d_rows);
    return hipGetLastError();
}
extern "C" hipError_t fx_launch_eval_list(const DevProblem *d_prob, const int64_t *d_ids, int64_t n, size_t lds_bytes, bool obst, bool extra,
                                          const EvalListRow *d_rows, int n_rows, int lanes, hipEvent_t ev_start, hipEvent_t ev_stop,
                                          hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (d_rows) {
        if (n_rows <= 0) return hipSuccess;
        if (extra && lanes != 1) return hipErrorInvalidValue;   // (windowed terms need the whole horizon in one lane)
#define FX_ROWS(G, O, E) return fx_launch_eval_list_rows<G, O, E>(d_rows, n_rows, n, lds_bytes, ev_start, ev_stop, stream)
        if (lanes == 1 && extra) { if (obst) FX_ROWS(1, true, true); FX_ROWS(1, false, true); }
        if (lanes == 1) { if (obst) FX_ROWS(1, true, false); FX_ROWS(1, false, false); }
        if (lanes == 8) { if (obst) FX_ROWS(8, true, false); FX_ROWS(8, false, false); }
        if (lanes == 32) { if (obst) FX_ROWS(32, true, false); FX_ROWS(32, false, false); }
#undef FX_ROWS
        return hipErrorInvalidValue;
    }
    const dim3 grid((unsigned)((n + FX_BLOCK - 1) / FX_BLOCK)), block(FX_BLOCK);
#define FX_LAUNCH(O, E)                                                                                         \
    do {                                                                                                        \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fx_eval_list_kernel<O, E>>(lds_bytes); e_ != hipSuccess) return e_; \
        hipExtLaunchKernelGGL((fx_eval_list_kernel<O, E>), grid, block, lds_bytes, stream, ev_start, ev_stop, 0, d_prob, d_ids); \
        return hipGetLastError();                                                                               \
    } while (0)
    if (obst && extra) FX_LAUNCH(true, true);
    if (obst) FX_LAUNCH(true, false);
    if (extra) FX_LAUNCH(false, true);
    FX_LAUNCH(false, false);
#undef FX_LAUNCH
}

// stable cost order of the candidates of n_agents agents (fx_sort_kernel.h): agents args->agent0 ... are grid.y, the largest of them
// (max_C candidates) chooses the decomposition.  The events, where given, bracket the whole launch sequence.
extern "C" hipError_t fx_launch_sort(const FxSortArgs *args, int n_agents, int64_t max_C, hipEvent_t ev_start, hipEvent_t ev_stop,
                                     hipStream_t stream) {
    if (n_agents <= 0 || max_C <= 0) return hipSuccess;
    hipError_t e;
    if (ev_start && (e = hipEventRecord(ev_start, stream)) != hipSuccess) return e;
    if (max_C <= FX_SORT_SMALL_MAX) {
        const size_t lds_bytes = FX_SORT_SMALL_LDS(max_C);
        if ((e = fx_allow_dynamic_lds<&fx_sort_small_kernel>(lds_bytes, FX_SORT_SMALL_LDS(FX_SORT_SMALL_MAX))) != hipSuccess) return e;
        hipLaunchKernelGGL(fx_sort_small_kernel, dim3(1, n_agents), dim3(FX_SORT_BLOCK), lds_bytes, stream, *args);
    } else {
        const dim3 tiles((unsigned)args->tiles_max, n_agents), one(1, n_agents), block(FX_SORT_BLOCK);
        hipLaunchKernelGGL(fx_sort_hist_kernel<true>, tiles, block, 0, stream, *args, 0);
        hipLaunchKernelGGL(fx_sort_scan_kernel<true>, one, block, 0, stream, *args);
        hipLaunchKernelGGL((fx_sort_scatter_kernel<true, false>), tiles, block, 0, stream, *args, 0);
        for (int pass = 1; pass < FX_SORT_PASSES; pass++) {
            hipLaunchKernelGGL(fx_sort_hist_kernel<false>, tiles, block, 0, stream, *args, pass);
            hipLaunchKernelGGL(fx_sort_scan_kernel<false>, one, block, 0, stream, *args);
            if (pass == FX_SORT_PASSES - 1) hipLaunchKernelGGL((fx_sort_scatter_kernel<false, true>), tiles, block, 0, stream, *args, pass);
            else hipLaunchKernelGGL((fx_sort_scatter_kernel<false, false>), tiles, block, 0, stream, *args, pass);
        }
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_stop && (e = hipEventRecord(ev_stop, stream)) != hipSuccess) return e;
    return hipSuccess;
}

// cost and flag word of n consecutive ranks of an order (fx_sort_gather_kernel)
extern "C" hipError_t fx_launch_sort_gather(const int64_t *d_order, int64_t n, const double *cost, const uint32_t *flags, int64_t C,
                                            unsigned long long *out_cost, uint32_t *out_flags, hipStream_t stream) {
    if (n > 0)
        hipLaunchKernelGGL(fx_sort_gather_kernel, dim3((unsigned)((n + FX_SORT_BLOCK - 1) / FX_SORT_BLOCK)), dim3(FX_SORT_BLOCK), 0, stream,
                           d_order, n, cost, flags, C, out_cost, out_flags);
    return hipGetLastError();
}

// A finished step re-scored under a->n_vec weight vectors (fx_rescore_kernel.h).  p: fx_rescore_plan of the
// call -- the regime, the partials per vector and the grids; the partials' buffers hold a->n_vec x p->n_part entries.  The totals, where
// asked for, come from the lane kernel in both regimes (coalesced stores): beside the vector kernel it runs without its reduction.
// ev_start / ev_stop bracket all launches.
extern "C" hipError_t fx_launch_rescore(const FxRescoreArgs *a, const FxRescorePlan *p, hipEvent_t ev_start, hipEvent_t ev_stop,
                                        hipStream_t stream) {
    hipError_t e;
    if (ev_start && (e = hipEventRecord(ev_start, stream)) != hipSuccess) return e;
    fxrs::Dims d{a->n, a->ld, a->n_cost, a->n_pred, a->deferred, a->n_vec, p->vec_chunk, p->n_part, p->per};
    const dim3 grid((unsigned)p->n_part, (unsigned)p->grid_y);
    if (p->regime == FX_RESCORE_LANE) {
        hipLaunchKernelGGL(fxrs::fx_rescore_lane_kernel<true>, grid, dim3(FX_RESCORE_TILE), 0, stream, a->costmap, a->flags, a->w, d, a->part_cost,
                           a->part_idx, a->totals);
    } else {
        hipLaunchKernelGGL(fxrs::fx_rescore_vector_kernel, grid, dim3(64), 0, stream, a->costmap, a->flags, a->w, d, a->part_cost, a->part_idx);
        if (a->totals && a->n > 0) {
            const FxRescorePlan t = fx_rescore_plan(a->n, a->n_vec, FX_RESCORE_LANE);
            d.vec_chunk = t.vec_chunk;
            hipLaunchKernelGGL(fxrs::fx_rescore_lane_kernel<false>, dim3((unsigned)t.n_part, (unsigned)t.grid_y), dim3(FX_RESCORE_TILE), 0, stream,
                               a->costmap, a->flags, a->w, d, nullptr, nullptr, a->totals);
        }
    }
    hipLaunchKernelGGL(fxrs::fx_rescore_finish_kernel, dim3((unsigned)p->finish_blocks), dim3(256), 0, stream, a->part_cost, a->part_idx, p->n_part,
                       a->n_vec, a->winner, a->cost);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_stop && (e = hipEventRecord(ev_stop, stream)) != hipSuccess) return e;
    return hipSuccess;
}

// A table of entries -- agents with their own weight vectors and effective cost lists -- re-scored in one call
// (fx_rescore_batch_kernel.h): the lane-regime entries' launch and the vector-regime entries' launch, each only
// where it has entries, and one finish launch with a wave per (entry, vector) -- three launches at most whatever the number of
// entries.  a->tot_entries: the entries whose totals the lane kernel writes without its reduction (vector-regime entries of the
// per-agent call that asked for totals), one more launch where there are any.  ev_start / ev_stop bracket all launches.
extern "C" hipError_t fx_launch_rescore_batch(const FxRescoreBatchArgs *a, hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t stream) {
    hipError_t e;
    if (ev_start && (e = hipEventRecord(ev_start, stream)) != hipSuccess) return e;
    const int n_all = a->n_lane + a->n_vector;
    if (a->n_lane > 0 && a->lane_wgs > 0)
        hipLaunchKernelGGL(fxrs::fx_rescore_batch_lane_kernel<true>, dim3((unsigned)a->lane_wgs), dim3(FX_RESCORE_TILE), 0, stream, a->entries,
                           a->wg0, a->n_lane);
    if (a->n_vector > 0 && a->vector_wgs > 0)
        hipLaunchKernelGGL(fxrs::fx_rescore_batch_vector_kernel, dim3((unsigned)a->vector_wgs), dim3(64), 0, stream, a->entries + a->n_lane,
                           a->wg0 + a->n_lane, a->n_vector);
    if (a->n_tot > 0 && a->tot_wgs > 0)
        hipLaunchKernelGGL(fxrs::fx_rescore_batch_lane_kernel<false>, dim3((unsigned)a->tot_wgs), dim3(FX_RESCORE_TILE), 0, stream, a->tot_entries,
                           a->tot_wg0, a->n_tot);
    if (a->finish_blocks > 0)
        hipLaunchKernelGGL(fxrs::fx_rescore_batch_finish_kernel, dim3((unsigned)a->finish_blocks), dim3(256), 0, stream, a->entries, a->wg0 + n_all,
                           n_all, a->n_waves);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev_stop && (e = hipEventRecord(ev_stop, stream)) != hipSuccess) return e;
    return hipSuccess;
}

// The obstacle stage of a finished step over the a->n_hyp prediction sets of one ROUND (fx_hypotheses_kernel.h; DESIGN.md section 25;
// rounds: fx_hypotheses_plan.h): items, finish, selection -- three launches.  lds_bytes = CH * K * 48 of an item's wave.  The caller
// records its events around the rounds of a call.
extern "C" hipError_t fx_launch_hypotheses(const FxHypArgs *a, size_t lds_bytes, hipStream_t stream) {
    const dim3 grid((unsigned)(a->n_tiles * a->NC), (unsigned)a->n_hyp);
#define FX_LAUNCH(CHv)                                                                                                       \
    if (a->CH == CHv) {                                                                                                      \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fxhy::fx_hyp_item_kernel<CHv>>(lds_bytes); e_ != hipSuccess) return e_; \
        hipLaunchKernelGGL(fxhy::fx_hyp_item_kernel<CHv>, grid, dim3(64), lds_bytes, stream, *a);                              \
    } else
    FX_LAUNCH(2) FX_LAUNCH(3) FX_LAUNCH(5) return hipErrorInvalidValue;
#undef FX_LAUNCH
    hipLaunchKernelGGL(fxhy::fx_hyp_finish_kernel, dim3((unsigned)a->n_part, (unsigned)a->n_hyp), dim3(FX_HYP_FINISH_TILE), 0, stream, *a);
    hipLaunchKernelGGL(fxhy::fx_hyp_select_kernel, dim3((unsigned)a->n_hyp), dim3(1024), 0, stream, *a);
    return hipGetLastError();
}

// The same for the rows of one ROUND of a call over several agents (fx_hypotheses_batch_kernel.h; rounds:
// fx_hypotheses_batch_plan.h): items, finish, selection over flat grids -- three launches whatever the number of agents.
// a->lds_bytes = CH * (largest K of the round's rows) * 48.  The caller records its events around the rounds of a call.
extern "C" hipError_t fx_launch_hypotheses_batch(const FxHypBatchArgs *a, hipStream_t stream) {
    if (a->n_rows < 1 || a->items < 1 || a->fin_blocks < 1 || a->pairs < 1 || a->items > FX_HYP_GRID_MAX || a->fin_blocks > FX_HYP_GRID_MAX ||
        a->pairs > FX_HYP_GRID_MAX)
        return hipErrorInvalidValue;
#define FX_LAUNCH(CHv)                                                                                                                  \
    if (a->CH == CHv) {                                                                                                                 \
        if (const hipError_t e_ = fx_allow_dynamic_lds<&fxhy::fx_hyp_batch_item_kernel<CHv>>(a->lds_bytes); e_ != hipSuccess) return e_; \
        hipLaunchKernelGGL(fxhy::fx_hyp_batch_item_kernel<CHv>, dim3((unsigned)a->items), dim3(64), a->lds_bytes, stream, a->rows, a->item0, \
                           a->n_rows);                                                                                                  \
    } else
    FX_LAUNCH(2) FX_LAUNCH(3) FX_LAUNCH(5) return hipErrorInvalidValue;
#undef FX_LAUNCH
    hipLaunchKernelGGL(fxhy::fx_hyp_batch_finish_kernel, dim3((unsigned)a->fin_blocks), dim3(FX_HYP_FINISH_TILE), 0, stream, a->rows, a->fin0,
                       a->n_rows);
    hipLaunchKernelGGL(fxhy::fx_hyp_batch_select_kernel, dim3((unsigned)a->pairs), dim3(1024), 0, stream, a->rows, a->sel0, a->n_rows);
    return hipGetLastError();
}
