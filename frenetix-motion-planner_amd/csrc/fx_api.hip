// fx_api.hip -- host side of libfxplan.so: the C-ABI declared in include/fxplan.h.
//
// A context owns (a) one pinned host staging buffer + one device arena for all per-step inputs, so a plan
// step is ONE H2D copy, (b) the per-candidate outputs (cost, flags, cost map, SoA bundle), (c) a pinned
// read-back block for the counters/winner, so a plan step is ONE small D2H copy.  All work is enqueued on the
// context's HIP stream; nothing synchronises until fx_finish().
#include "fx_pass.h"

thread_local char g_err[512] = "";

// Time-bounded wait for a sequence word the device publishes into pinned host memory.  The reference bounds every hand-off
// between its processes with TIMEOUT = 20 s (cr_scenario_handler/simulation/simulation.py:637,655, agent_batch.py:98): a
// peer that never joins a collective, or a faulted kernel, must surface as an error, not as a hang.  Pure host code.
extern "C" int32_t fx_wait_word(const volatile unsigned long long *word, unsigned long long expected, int32_t timeout_ms) {
    if (!word) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_wait_word: NULL argument");
    for (int spin = 0; spin < 4096; spin++)
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == expected) return FX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const auto limit = std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms);
    for (;;) {
        for (int spin = 0; spin < 1024; spin++)
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == expected) return FX_OK;
        if (std::chrono::steady_clock::now() - t0 >= limit)
            return set_err(FX_ERR_TIMEOUT, "no answer from the device within %d ms (a peer that never joined the collective, or a "
                           "faulted kernel)", timeout_ms);
    }
}

extern "C" {


int32_t fx_abi_version(void) { return FX_ABI_VERSION; }
const char *fx_last_error(void) { return g_err; }

int32_t fx_device_count(int32_t *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return set_err(FX_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return FX_OK;
}

int32_t fx_create_batch(FxContext **out, int32_t device, int32_t max_agents, int64_t max_candidates_total,
                        int32_t max_steps, int32_t max_ref_knots, int32_t max_obstacles, int32_t max_pred_steps) {
    if (out) *out = nullptr;   // and it stays NULL unless everything below succeeds: the owners give back what a failed create had built
    if (!out || max_candidates_total < 1 || max_steps < 1 || max_steps + 1 > FX_MAX_SAMPLES || max_ref_knots < 2 ||
        max_agents < 1 || max_obstacles < 0 || max_pred_steps < 0)
        return set_err(FX_ERR_INVALID_ARGUMENT, "fx_create: bad capacity arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return set_err(FX_ERR_NO_DEVICE, "no HIP device visible");
    }
    if (device < 0 || device >= ndev) return set_err(FX_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<FxContext> ctx(new (std::nothrow) FxContext());
    FxContext *c = ctx.get();
    if (!c) return set_err(FX_ERR_HIP, "out of host memory");
    c->device = device;
    c->caps = fx_caps_of(max_agents, max_candidates_total, max_steps, max_ref_knots, max_obstacles, max_pred_steps);
    c->max_agents = max_agents;
    {   // FX_STREAM_PRIORITY=low|high: experiments with two contexts sharing the device (tools/ns_two_streams.py)
        const char *pr = getenv("FX_STREAM_PRIORITY");
        int least = 0, greatest = 0;
        const bool with_priority = pr && *pr && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
        const int priority = pr && pr[0] == 'l' ? least : greatest;
        FX_TRY(c->stream.create(with_priority ? &priority : nullptr));
    }
    for (auto &t : c->ring)
        for (FxEvent *e : {&t.e0, &t.e_eval, &t.e_end, &t.e_obs0, &t.e_obs1}) FX_TRY(e->create());
    const int S = max_steps + 1;
    const size_t total_ld = (size_t)c->caps.total_ld, A = (size_t)max_agents;
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    c->in_bytes = A * input_bytes_for(0, S, max_ref_knots, max_obstacles, c->caps.max_pred, false) +
                  align_up(sizeof(double) * 13 * (size_t)max_candidates_total, 256) + 4096;
    c->probs_bytes = align_up(sizeof(DevProblem) * A, 256);
    c->in_bytes += c->probs_bytes;
    FX_TRY(c->h_in.alloc(c->in_bytes, hipHostMallocMapped));
    if (const char *sm = getenv("FX_STAGE")) c->stage_mode = !strcmp(sm, "dma") ? 1 : (!strcmp(sm, "kernel") ? 2 : (!strcmp(sm, "bar") ? 3 : 0));
    if (const char *of = getenv("FX_OBST_STAGE")) c->force.obst_stage = std::max(0, std::min(2, atoi(of)));   // experiments: fx_set_obstacle_stage's first argument
    FX_TRY(c->d_in.alloc(c->in_bytes));
    if (c->stage_mode == 3) {   // opt-in (see probe_host_writes)
        c->bar_ok = probe_host_writes(c, device, c->d_in, c->in_bytes);
        if (!c->bar_ok)
            return set_err(FX_ERR_HIP, "FX_STAGE=bar: the device memory of GPU %d is not host-writable from this process, has no HDP flush "
                           "register, or a kernel did not see a rewritten line", device);
    }
    c->h_probs = reinterpret_cast<DevProblem *>(c->h_in.get());
    c->d_probs = reinterpret_cast<DevProblem *>(c->d_in.get());
    FX_TRY(c->d_cost.alloc(total_ld));
    FX_TRY(c->d_cost_tail.alloc(total_ld));
    FX_TRY(c->d_flags.alloc(total_ld));
    FX_TRY(c->d_costmap.alloc((size_t)FX_NUM_COSTS * total_ld));
    FX_TRY(c->d_coeffs.alloc((size_t)FX_COEFF_ROWS * total_ld));
    FX_TRY(c->d_trajlen.alloc(total_ld));
    FX_TRY(c->d_bstep.alloc(total_ld));
    FX_TRY(c->d_part_cost.alloc(c->caps.max_blocks_total));
    FX_TRY(c->d_part_idx.alloc(c->caps.max_blocks_total));
    FX_TRY(c->d_counters.alloc(A * FX_CNT_COUNT));
    FX_TRY(c->h_counters.alloc(A * (FX_CNT_COUNT + 1), mapped));
    memset(c->h_counters, 0, sizeof(unsigned long long) * A * (FX_CNT_COUNT + 1));
    // ON THE CONTEXT'S STREAM: hipMemset on device memory runs on the null stream and may return before it has executed, and
    // a non-blocking stream does not wait for the null stream -- on a busy GPU (a second process) the zeroing landed behind the
    // first step's counter atomics and the step published zeros (tests/test_soak_parity.py, once in a few hundred contexts)
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long) * A * FX_CNT_COUNT, c->stream));
    FX_TRY(c->d_bar.alloc(2 * 16 * 65));   // (two barrier blocks: fx_step_kernel.h, FX_BAR_WORDS)
    HIP_TRY(hipMemsetAsync(c->d_bar, 0, sizeof(unsigned long long) * 2 * 16 * 65, c->stream));
    if (const char *e = getenv("FX_STEP_KERNEL")) c->force.step_kernel = atoi(e) ? 2 : 1;
    FX_TRY(c->h_pub.alloc(FX_PUB_MAX + 1, mapped));
    memset(c->h_pub, 0, sizeof(double) * (FX_PUB_MAX + 1));
    FX_TRY(c->d_topk_cost.alloc(A * 64));
    FX_TRY(c->d_topk_idx.alloc(A * 64));
    FX_TRY(c->d_topk_scr_cost.alloc(A * 64 * 64));
    FX_TRY(c->d_topk_scr_idx.alloc(A * 64 * 64));
    FX_TRY(c->h_topk_cost.alloc(A * 64, hipHostMallocDefault));
    c->pkg_plane_rows = FX_NUM_PLANES * (max_steps + 1);
    c->pkg_stride = (c->pkg_plane_rows + FX_PKG_TAIL + 1 + 7) & ~7;
    FX_TRY(c->h_pkg.alloc(A * c->pkg_stride, mapped));
    memset(c->h_pkg, 0, sizeof(double) * A * c->pkg_stride);
    FX_TRY(c->d_winner_own.alloc(A * 2));
    FX_TRY(c->h_cand.alloc((size_t)FX_NUM_PLANES * (max_steps + 1) + FX_COEFF_ROWS + FX_NUM_COSTS + 4, hipHostMallocDefault));
    FX_TRY(c->h_topk_idx.alloc(A * 64, hipHostMallocDefault));
    c->slots.resize(max_agents);
    c->plan_rows.resize(max_agents);
    c->plan.agents = c->plan_rows.data();
    *out = ctx.release();
    return FX_OK;
}

int32_t fx_create(FxContext **out, int32_t device, int64_t max_candidates, int32_t max_steps, int32_t max_ref_knots,
                  int32_t max_obstacles, int32_t max_pred_steps) {
    return fx_create_batch(out, device, 1, max_candidates, max_steps, max_ref_knots, max_obstacles, max_pred_steps);
}

int32_t fx_destroy(FxContext *c) {
    if (!c) return FX_OK;
    // a context whose wait timed out may hold work that never finishes (a collective a peer never joined): freeing its buffers
    // or its communicator would wait for that work.  It is abandoned as it is; the process is expected to end.
    if (c->timed_out) return FX_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)fx_comm_destroy(c);
    delete c;   // every member gives back what it holds (fx_owner.h), the stream last
    return FX_OK;
}

// Publish n doubles of a device buffer (e.g. the all-gathered survivors) to the host through pinned memory;
// enqueued on the context stream.  fx_wait_published copies them out once they have arrived.
int32_t fx_publish(FxContext *c, const void *d_src, int32_t n) {
    if (!c || !d_src) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_publish: NULL argument");
    if (n < 1 || n > FX_PUB_MAX) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_publish: n=%d outside [1,%d]", n, FX_PUB_MAX);
    HIP_TRY(hipSetDevice(c->device));
    c->pub_seq++;
    c->pub_n = n;
    HIP_TRY(fx_launch_publish(reinterpret_cast<const double *>(d_src), n, c->h_pub.dev,
                              reinterpret_cast<unsigned long long *>(c->h_pub.dev + FX_PUB_MAX), c->pub_seq, c->stream));
    c->in_flight = true; c->tail_work = true;
    return FX_OK;
}

int32_t fx_wait_published(FxContext *c, double *out) {
    if (!c || !out) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_wait_published: NULL argument");
    if (c->pub_n < 1) return set_err(FX_ERR_NOT_READY, "nothing published");
    int rc = wait_seq(c, reinterpret_cast<const unsigned long long *>(c->h_pub + FX_PUB_MAX), c->pub_seq);
    if (rc) return rc;
    memcpy(out, c->h_pub, sizeof(double) * c->pub_n);
    return FX_OK;
}


int32_t fx_set_timeout_ms(FxContext *c, int32_t timeout_ms) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (timeout_ms < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "timeout must be at least 1 ms");
    c->timeout_ms = timeout_ms;
    return FX_OK;
}

int32_t fx_set_winner_buffer(FxContext *c, void *d_winner) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    c->dev_winner = reinterpret_cast<double *>(d_winner);
    return FX_OK;
}

int32_t fx_set_store_mode(FxContext *c, int32_t store_mode) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (store_mode < 0 || store_mode > 2) return set_err(FX_ERR_INVALID_ARGUMENT, "store mode must be 0 (auto), 1 (write-back) or 2 (write-through)");
    c->force.store = store_mode;
    return FX_OK;
}

int32_t fx_set_part_mapping(FxContext *c, int32_t mapping) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (mapping < 0 || mapping > 2) return set_err(FX_ERR_INVALID_ARGUMENT, "mapping must be 0 (auto), 1 (lane split) or 2 (wave split)");
    c->force.wsplit = mapping;
    return FX_OK;
}

int32_t fx_set_block_size(FxContext *c, int32_t block_size) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (block_size != 0 && block_size != 64 && block_size != 128 && block_size != 256)
        return set_err(FX_ERR_INVALID_ARGUMENT, "block_size must be 0 (auto), 64, 128 or 256");
    c->force.block = block_size;
    return FX_OK;
}

int32_t fx_set_tuning(FxContext *c, int32_t lanes_per_candidate, int32_t waves_per_simd, int32_t kernel_variant) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (lanes_per_candidate != 0 && lanes_per_candidate != 1 && lanes_per_candidate != 2 && lanes_per_candidate != 4 &&
        lanes_per_candidate != 8 && lanes_per_candidate != 16 && lanes_per_candidate != 32)
        return set_err(FX_ERR_INVALID_ARGUMENT, "lanes_per_candidate must be 0 (auto), 1, 2, 4, 8, 16 or 32");
    if (waves_per_simd != 0 && (waves_per_simd < 2 || waves_per_simd > 4))
        return set_err(FX_ERR_INVALID_ARGUMENT, "waves_per_simd must be 0 (auto), 2, 3 or 4");
    if (kernel_variant < 0 || kernel_variant > 2) return set_err(FX_ERR_INVALID_ARGUMENT, "kernel_variant must be 0 (auto), 1 (generic) or 2 (grid)");
    c->force.G = lanes_per_candidate;
    c->force.wpe = waves_per_simd;
    c->force.variant = kernel_variant;
    return FX_OK;
}

int32_t fx_set_stream(FxContext *c, void *hip_stream) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    c->stream.borrow(reinterpret_cast<hipStream_t>(hip_stream));
    c->user_stream = c->tail_work = true;   // (whatever else the caller queues on it may read the arena: no host writes, ever)
    return FX_OK;
}

int64_t fx_device_bytes(const FxContext *c) { return c ? c->dev_bytes : 0; }
double fx_last_kernel_ms(const FxContext *cc) {
    FxContext *c = const_cast<FxContext *>(cc);
    if (!c || !c->evaluated || c->n_timed == 0) return 0.0;
    FxContext::TimeSlot &t = c->ring[(c->n_timed - 1) % FxContext::kTimeRing];
    return fetch_slot(c, t) ? 0.0 : (double)t.step_ms;
}
double fx_last_eval_kernel_ms(const FxContext *cc) {
    FxContext *c = const_cast<FxContext *>(cc);
    if (!c || !c->evaluated || c->n_timed == 0) return 0.0;
    FxContext::TimeSlot &t = c->ring[(c->n_timed - 1) % FxContext::kTimeRing];
    return fetch_slot(c, t) ? 0.0 : (double)t.eval_ms;
}
int32_t fx_read_kernel_times(FxContext *c, int32_t max_n, double *eval_ms, double *step_ms, int32_t *n_out) {
    if (!c || max_n < 0 || !n_out) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_read_kernel_times: bad argument");
    const long long have = std::min<long long>(c->n_timed, FxContext::kTimeRing);
    const int n = (int)std::min<long long>(have, max_n);
    for (int k = 0; k < n; k++) {  // oldest of the returned window first
        FxContext::TimeSlot &t = c->ring[(c->n_timed - n + k) % FxContext::kTimeRing];
        int rc = fetch_slot(c, t);
        if (rc) return rc;
        if (eval_ms) eval_ms[k] = t.eval_ms;
        if (step_ms) step_ms[k] = t.step_ms;
    }
    *n_out = n;
    return FX_OK;
}
int32_t fx_set_timing_interval(FxContext *c, int32_t every) {
    if (!c || every < 1) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_set_timing_interval: every=%d", every);
    c->timing_every = every;
    return FX_OK;
}
// How the last evaluation was launched (tests and tools): out[0] grid kernel, [1] lanes per candidate, [2] waves per SIMD,
// [3] workgroup size, [4] wave split, [5] fused selection, [6] workgroups per agent (max), [7] agents, [8] winner package,
// [9] dynamic LDS bytes
int32_t fx_step_info(const FxContext *c, int64_t *out10) {
    if (!c || !out10) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_step_info: NULL argument");
    int64_t v[16];
    fx_step_info_of(c->plan, c->launch, c->stage_path, v);
    memcpy(out10, v, sizeof(int64_t) * 10);
    return FX_OK;
}

int32_t fx_set_obstacle_stage(FxContext *c, int32_t stage, int32_t steps_per_item) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (stage < 0 || stage > 2) return set_err(FX_ERR_INVALID_ARGUMENT, "stage must be 0 (auto), 1 (fused into the walk) or 2 (own kernel)");
    if (steps_per_item != 0 && steps_per_item != 2 && steps_per_item != 3 && steps_per_item != 5)
        return set_err(FX_ERR_INVALID_ARGUMENT, "steps_per_item must be 0 (auto), 2, 3 or 5");
    c->force.obst_stage = stage; c->force.obst_CH = steps_per_item;
    return FX_OK;
}
double fx_last_obstacle_kernel_ms(const FxContext *cc) {
    FxContext *c = const_cast<FxContext *>(cc);
    if (!c || !c->evaluated || c->n_timed == 0) return 0.0;
    FxContext::TimeSlot &t = c->ring[(c->n_timed - 1) % FxContext::kTimeRing];
    return fetch_slot(c, t) ? 0.0 : (double)t.obst_ms;
}
int32_t fx_read_obstacle_kernel_times(FxContext *c, int32_t max_n, double *obst_ms, int32_t *n_out) {
    if (!c || max_n < 0 || !n_out) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_read_obstacle_kernel_times: bad argument");
    const long long have = std::min<long long>(c->n_timed, FxContext::kTimeRing);
    const int n = (int)std::min<long long>(have, max_n);
    for (int k = 0; k < n; k++) {  // oldest of the returned window first
        FxContext::TimeSlot &t = c->ring[(c->n_timed - n + k) % FxContext::kTimeRing];
        int rc = fetch_slot(c, t);
        if (rc) return rc;
        if (obst_ms) obst_ms[k] = t.obst_ms;
    }
    *n_out = n;
    return FX_OK;
}
// fx_step_info, extended: out[0 .. 9] as fx_step_info, [10] obstacle stage as its own kernel, [11] steps per work item, [12] work
// items (waves) per agent (max) and [13] dynamic LDS bytes of that kernel, [14] waves per workgroup when a tile's chunks share one
// workgroup (0: one wave per (tile, chunk) item), [15] what the agent's last workgroup did beyond the arg-min (1: collision count,
// 2: winner package; fx_tail.h)
int32_t fx_step_info_ex(const FxContext *c, int64_t *out16) {
    if (!c || !out16) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_step_info_ex: NULL argument");
    fx_step_info_of(c->plan, c->launch, c->stage_path, out16);
    return FX_OK;
}

int32_t fx_set_step_kernel(FxContext *c, int32_t mode, int32_t steps_per_item) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (mode < 0 || mode > 2) return set_err(FX_ERR_INVALID_ARGUMENT, "mode must be 0 / 1 (off: three launches) or 2 (on where applicable)");
    if (steps_per_item != 0 && steps_per_item != 3 && steps_per_item != 5 && steps_per_item != 8)
        return set_err(FX_ERR_INVALID_ARGUMENT, "steps_per_item must be 0 (auto), 3, 5 or 8");
    c->force.step_kernel = mode; c->force.step_kernel_CH = steps_per_item;   // (the mode takes effect at the next upload)
    return FX_OK;
}
int32_t fx_set_fused_selection(FxContext *c, int32_t enabled) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    c->force.fuse_enabled = enabled != 0;
    c->force.fuse_any_size = enabled == 2;   // (takes effect at the next upload)
    return FX_OK;
}
int32_t fx_set_timing(FxContext *c, int32_t mode) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (mode < FX_TIMING_OFF || mode > FX_TIMING_KERNEL) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_set_timing: unknown mode");
    c->timing = mode;
    return FX_OK;
}

// device pointers of agent 0's outputs, for callers that keep working on the GPU (torch tensors via
// from_blob-style wrapping or RCCL sends): cost f64[ld], flags u32[ld], planes f64[14][S][ld]
int32_t fx_device_views(FxContext *c, int32_t agent, void **cost, void **flags, void **planes, int64_t *ld) {
    int rc = check_agent(c, agent);
    if (rc) return rc;
    if (cost) *cost = c->h_probs[agent].cost;
    if (flags) *flags = c->h_probs[agent].flags;
    if (planes) *planes = (c->slots[agent].mode & FX_MODE_WRITE_BUNDLE) ? c->h_probs[agent].planes : nullptr;
    if (ld) *ld = c->slots[agent].ld;
    return FX_OK;
}

}  // extern "C"
