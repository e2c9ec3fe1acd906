// fx_api_step.hip -- the plan step through the C-ABI: upload, fx_evaluate (launch policy: fx_policy.h), results, state
// updates, the winner package and the batched plan calls (header: include/fxplan.h; context: fx_context.h).
#include "fx_pass.h"

// the derived columns of planner.py:394-447 (_compute_trajectory_pair) behind the FX_NUM_PLANES planes of a package block: yaw rate by
// backward differences of the heading, steering angle of the kinematic single-track model, heading shifted into
// [x0_orientation - pi, x0_orientation + pi]
void fx_package_derive(const DevProblem &d, int S, double yaw_rate0, double *block) {
    const double *theta = block + 2 * (size_t)S, *kappa = block + 5 * (size_t)S;
    double *yaw = block + (size_t)FX_NUM_PLANES * S, *steer = yaw + S, *orient = steer + S;
    const double lo = d.x0_orientation - M_PI, hi = d.x0_orientation + M_PI, wb = d.veh.wheelbase;
    for (int i = 0; i < S; i++) {
        yaw[i] = i == 0 ? yaw_rate0 : (theta[i] - theta[i - 1]) / d.dt;
        steer[i] = std::atan2(wb * kappa[i], 1.0);
        double o = theta[i];
        for (int r = 0; r < 4; r++) {
            if (o < lo) o += 2 * M_PI;
            if (o > hi) o -= 2 * M_PI;
        }
        orient[i] = o;
    }
}

extern "C" {

// the range [lo, hi) of the pinned staging block, brought to the device arena: host writes, the staging kernel or the DMA engine
// (small ranges through the staging kernel: the DMA engine's submission latency dominates below ~1 MiB; offsets inside the block
// are multiples of 256, so the 16-byte lanes of the staging kernel line up)
static int stage_range(FxContext *c, size_t lo, size_t hi) {
    const size_t lo16 = lo & ~(size_t)15, hi16 = (hi + 15) & ~(size_t)15;
    // host writes only while nothing of this context is in flight: fx_update_state drained the stream (or fx_finish saw the
    // previous step's last word) before the block was rewritten, so no kernel still reads the arena
    if (hi16 <= c->in_bytes && host_stage_allowed(c, hi16 - lo16))
        host_stage(c, lo16, hi16);
    else if (c->stage_mode == 2 || (c->stage_mode != 1 && hi16 - lo16 <= FX_STAGE_KERNEL_MAX && hi16 <= c->in_bytes)) {
        HIP_TRY(fx_launch_stage(c->h_in.dev + lo16, c->d_in + lo16, hi16 - lo16, c->stream));
        c->stage_path = 2;
    } else {
        HIP_TRY(hipMemcpyAsync(c->d_in + lo, c->h_in + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
        c->stage_path = 1;
    }
    return FX_OK;
}

// Stage n_agents problems.  Agent a's candidates occupy [cand_off, cand_off + ld) of every per-candidate array.
int32_t fx_upload_batch(FxContext *c, int32_t n_agents, const FxProblem *probs) {
    if (!c || !probs) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_upload: NULL argument");
    if (n_agents < 1 || n_agents > c->max_agents) return set_err(FX_ERR_CAPACITY, "n_agents=%d exceeds capacity %d", n_agents, c->max_agents);
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out (its stream may never drain): destroy it");
    HIP_TRY(hipSetDevice(c->device));
    if (c->in_flight) {  // the pinned staging block is about to be rewritten: earlier copies must have landed
        FX_TRY(fx_drain(c));
        c->in_flight = false;
    }
    c->uploaded = c->evaluated = false;
    for (int a = 0; a < n_agents; a++) {
        int rc = validate(&probs[a]);
        if (rc) return rc;
    }
    // how the step runs (fx_policy.h); experiments: occupancy cap through LDS, bound of the in-kernel collision count
    static const int64_t tail_max_c = [] { const char *e = getenv("FX_TAIL_MAX_C"); return e ? (int64_t)atoll(e) : FxForce().tail_max_c; }();
    const char *pad = getenv("FX_LDS_PAD");
    c->force.lds_pad = pad ? (size_t)atol(pad) : 0;
    c->force.tail_max_c = tail_max_c;
    // (experiment: FX_OBST_WG = 0 / 1 forces the obstacle kernel's single-wave items / workgroups; read with the upload, as the two
    // above, so that an evaluation puts no environment look-up in front of its first launch)
    const char *wg_env = getenv("FX_OBST_WG");
    c->force.obst_wg = wg_env ? (atoi(wg_env) ? 2 : 1) : 0;
    const char *ci_env = getenv("FX_OBST_CHUNK_INDEX");   // (test hook: tests/test_chunk_placement.py)
    c->force.obst_chunk_index = ci_env && atoi(ci_env) != 0;
    FxStepPlan &pl = c->plan;
    int rc = fx_plan_upload(n_agents, probs, c->force, c->caps, &pl, g_err, sizeof(g_err));
    if (rc) return rc;
    // the buffers the plan asks for, grown on demand
    // road boundary and the lanelets of the lane_center_offset cost: their own staging block (maps differ by orders of magnitude in size)
    size_t bound_need = 0;
    for (int a = 0; a < n_agents; a++) {
        const FxProblem *p = &probs[a];
        if (fx_has_boundary(p))
            bound_need += align_up(sizeof(double) * 4 * (size_t)p->n_bound, 256) + align_up(sizeof(int32_t) * ((size_t)p->M + 1), 256) +
                          align_up(sizeof(int32_t) * (size_t)p->bound_bin[p->M], 256);
        if (p->n_lane > 0)
            bound_need += align_up(sizeof(double) * 4 * (size_t)p->n_lane, 256) + 2 * align_up(sizeof(int32_t) * ((size_t)p->n_lane + 1), 256) +
                          align_up(sizeof(double) * 2 * (size_t)p->lane_poly_off[p->n_lane], 256) +
                          align_up(sizeof(double) * 2 * (size_t)p->lane_ctr_off[p->n_lane], 256);
    }
    if (bound_need > std::min(c->h_bound.size(), c->d_bound.size())) {
        const size_t cap = std::max<size_t>(2 * bound_need, 64 * 1024);
        FX_TRY(c->h_bound.ensure(cap, hipHostMallocDefault));
        FX_TRY(c->d_bound.ensure(cap));
    }
    FX_TRY(c->d_planes.ensure(pl.planes_bytes / sizeof(double)));
    if (pl.obs_part_n) {   // scratch of the obstacle kernel: tickets start (and are left) zeroed
        if (pl.obs_part_n > c->d_obs_part.size() || pl.obs_colm_n > c->d_obs_colm.size()) {   // both anew, at this step's sizes
            FX_TRY(fx_drain(c));
            c->d_obs_part.release(); c->d_obs_colm.release();
            FX_TRY(c->d_obs_part.alloc(pl.obs_part_n));
            FX_TRY(c->d_obs_colm.alloc(pl.obs_colm_n));
        }
        if (!c->d_obs_ticket) {
            const size_t n_tick = (size_t)(c->caps.total_ld / 64) + (size_t)c->max_agents;
            FX_TRY(c->d_obs_ticket.alloc(n_tick));
            HIP_TRY(hipMemsetAsync(c->d_obs_ticket, 0, sizeof(unsigned int) * n_tick, c->stream));   // (in order with the step's kernels)
        }
        if (!c->d_obs_list) FX_TRY(c->d_obs_list.alloc((size_t)c->caps.total_ld));
    }
    // the bytes, and every agent's DevProblem from its row of the plan
    Arena ar{c->h_in, c->d_in, c->probs_bytes, c->in_bytes};
    Arena br{c->h_bound, c->d_bound, 0, c->d_bound.size()};
    for (int a = 0; a < n_agents; a++) {
        const FxProblem *p = &probs[a];
        const FxAgentPlan &r = pl.agents[a];
        const int S = p->N + 1;
        DevProblem &d = c->h_probs[a];
        memset(&d, 0, sizeof(d));
        d.N = p->N; d.S = S; d.mode = r.mode; d.low_vel_mode = p->low_vel_mode; d.dt = p->dt;
        memcpy(d.x0_lon, p->x0_lon, sizeof(d.x0_lon));
        memcpy(d.x0_lat, p->x0_lat, sizeof(d.x0_lat));
        d.x0_orientation = p->x0_orientation; d.v_des = p->v_des; d.veh = p->veh;
        d.nT = p->nT; d.nV = p->nV; d.nD = p->nD; d.has_matrix = p->sampling_matrix != nullptr;
        d.lon_mode = p->lon_mode;
        d.C = r.C; d.g_base = r.g_base; d.ld = r.ld; d.M = p->M; d.K = p->K; d.P = p->P; d.n_cost = p->n_cost; d.n_dto = p->n_dto;
        for (int n = 0; n < p->n_cost; n++) {
            d.cost_id[n] = p->cost_id[n];
            d.cost_w[n] = p->cost_w[n];
        }
        memcpy(d.simpson_corr, p->simpson_corr, sizeof(d.simpson_corr));
        bool ok = true;
        FxAgentSlot &sl = c->slots[a];
        sl = FxAgentSlot();
        sl.nT = p->nT; sl.nV = p->nV; sl.nD = p->nD; sl.K = p->K; sl.P = p->P; sl.M = p->M;
        sl.want_collision = (p->mode & FX_MODE_COLLISION) != 0;
        // what may change from step to step (fx_update_state) comes first, right behind the problems, so that an update is
        // one copy of the front of the block; the per-reference constants follow
        if (d.has_matrix) {
            d.matrix = ar.put(p->sampling_matrix, (size_t)13 * fx_candidates_global(p), &ok);
        } else {
            sl.off_t = ar.off; d.t_samp = ar.put(p->t_samp, p->nT, &ok);
            sl.off_v = ar.off; d.v_samp = ar.put(p->v_samp, p->nV, &ok);
            sl.off_d = ar.off; d.d_samp = ar.put(p->d_samp, p->nD, &ok);
        }
        double *rec = nullptr, *hot = nullptr;
        unsigned long long *pm = nullptr, *hm = nullptr;
        const bool have_hull = p->K > 0 && p->obs_hull && p->obs_nhull;
        if (p->K > 0) {
            sl.have_hull = have_hull;
            // step-major packed records + per-step obstacle masks + hot table (filled below, once the knots are staged): what the
            // walk reads every step comes first, so that a state update stages this range only
            const double *dev = nullptr, *dhot = nullptr;
            const unsigned long long *dpm = nullptr, *dhm = nullptr;
            sl.off_rec = ar.off; rec = ar.host_slot<double>((size_t)S * p->K * 12, &dev, &ok);
            sl.off_pm = ar.off; pm = ar.host_slot<unsigned long long>((size_t)S * mask_words(p->K), &dpm, &ok);
            sl.off_hm = ar.off; hm = ar.host_slot<unsigned long long>((size_t)S * mask_words(p->K), &dhm, &ok);
            sl.off_hot = ar.off; hot = ar.host_slot<double>((size_t)S * p->K * FX_HOT_STRIDE, &dhot, &ok);
            d.obs_rec = dev; d.obs_pmask = dpm; d.obs_hmask = dhm; d.obs_hot = dhot;
            sl.dyn_end = ar.off;
            // the raw predictions: kept for re-packing; read on the device only by the lane parts of a candidate that start behind
            // the step at which it left the projection domain (finish_candidate: more than one lane per candidate, obstacle stage
            // inside the walk) -- fx_update_state stages them for such a plan
            sl.off_pos = ar.off; d.obs_pos = ar.put(p->obs_pos, (size_t)2 * p->K * p->P, &ok);
            sl.off_cov = ar.off; d.obs_cov_inv = ar.put(p->obs_cov_inv, (size_t)4 * p->K * p->P, &ok);
            sl.off_npred = ar.off; d.obs_npred = ar.put(p->obs_npred, p->K, &ok);
            sl.raw_end = ar.off;
            if (have_hull) {  // kept in the staging block for re-packing; the kernels read the hulls from `rec`
                sl.off_hull = ar.off; d.obs_hull = ar.put(p->obs_hull, (size_t)6 * p->K * (p->P - 1), &ok);
                sl.off_nhull = ar.off; d.obs_nhull = ar.put(p->obs_nhull, p->K, &ok);
            }
        } else {
            sl.dyn_end = ar.off;
        }
        d.tpow = ar.put(p->tpow, (size_t)5 * S, &ok);
        {   // reference knots, AoS: pos, theta, curv, curv_d, x, y, nx, ny
            const double *dev = nullptr;
            sl.off_ref = ar.off;
            double *h = ar.host_slot<double>((size_t)p->M * FX_REF_FIELDS, &dev, &ok);
            if (h) {
                for (int k = 0; k < p->M; k++) {
                    double *q = h + (size_t)k * FX_REF_FIELDS;
                    q[0] = p->ref_pos[k]; q[1] = p->ref_theta[k]; q[2] = p->ref_curv[k]; q[3] = p->ref_curv_d[k];
                    q[4] = p->ref_x[k]; q[5] = p->ref_y[k]; q[6] = p->ref_nx[k]; q[7] = p->ref_ny[k];
                }
                if (rec && pm && hm && hot) {
                    hot_origin_of(h, p->M, p->x0_lon[0], d.hot_origin);
                    d.hot_gap_margin = pack_obstacle_tables(S, p->K, p->P, p->obs_pos, p->obs_cov_inv, p->obs_npred, p->obs_hull,
                                                            p->obs_nhull, have_hull, d.hot_origin[0], d.hot_origin[1], rec, pm, hm, hot);
                }
            }
            d.ref = dev;
        }
        if (p->n_dto > 0) d.dto_pos = ar.put(p->dto_pos, (size_t)2 * p->n_dto, &ok);
        if (fx_has_boundary(p)) {
            d.n_bound = p->n_bound;
            d.bound_piece = br.put(p->bound_piece, (size_t)4 * p->n_bound, &ok);
            d.bound_bin = br.put(p->bound_bin, (size_t)p->M + 1, &ok);
            d.bound_item = br.put(p->bound_item, (size_t)p->bound_bin[p->M], &ok);
            d.bound_d_reach = p->bound_d_reach;
        }
        if (p->n_lane > 0) {
            d.n_lane = p->n_lane;
            d.lane_bbox = br.put(p->lane_bbox, (size_t)4 * p->n_lane, &ok);
            d.lane_poly_off = br.put(p->lane_poly_off, (size_t)p->n_lane + 1, &ok);
            d.lane_poly = br.put(p->lane_poly, (size_t)2 * p->lane_poly_off[p->n_lane], &ok);
            d.lane_ctr_off = br.put(p->lane_ctr_off, (size_t)p->n_lane + 1, &ok);
            d.lane_ctr = br.put(p->lane_ctr, (size_t)2 * p->lane_ctr_off[p->n_lane], &ok);
        }
        if (!ok) return set_err(FX_ERR_CAPACITY, "input arena too small (%zu bytes)", c->in_bytes);
        d.cost = c->d_cost + r.cand_off;
        d.cost_tail = c->d_cost_tail + r.cand_off;
        d.flags = c->d_flags + r.cand_off;
        d.costmap = c->d_costmap + (size_t)FX_NUM_COSTS * r.cand_off;  // [n_cost][ld] inside this agent's slab
        d.coeffs = c->d_coeffs + (size_t)FX_COEFF_ROWS * r.cand_off;
        d.traj_len = c->d_trajlen + r.cand_off;
        d.bound_step = c->d_bstep + r.cand_off;
        d.n_blocks = r.n_blocks;
        if (r.deferred) {
            d.obs_part = c->d_obs_part + r.obs_part_off;
            d.obs_colm = c->d_obs_colm + r.obs_colm_off;
            d.obs_ticket = c->d_obs_ticket + r.obs_tick_off;
            d.obs_list = c->d_obs_list + r.cand_off;   // the agent's slab of the per-candidate arrays
        }
        d.part_cost = c->d_part_cost + r.block_off;
        d.part_idx = c->d_part_idx + r.block_off;
        d.counters = c->d_counters + (size_t)a * FX_CNT_COUNT;
        d.pkg_out = c->h_pkg.dev + (size_t)a * c->pkg_stride;
        d.pkg_seq = reinterpret_cast<unsigned long long *>(d.pkg_out + c->pkg_stride - 1);
        d.pkg_plane_rows = c->pkg_plane_rows;
        if (r.mode & FX_MODE_WRITE_BUNDLE) d.planes = c->d_planes + r.planes_off / sizeof(double);
        sl.C = r.C; sl.ld = r.ld; sl.cand_off = r.cand_off; sl.S = S; sl.n_cost = p->n_cost; sl.n_blocks = r.n_blocks; sl.mode = r.mode;
    }
    c->last_live = -1;
    c->n_agents = n_agents;
    c->in_used = ar.off;
    c->dirty_lo = (size_t)-1; c->dirty_hi = 0; c->probs_dirty = false;
    if ((rc = stage_range(c, 0, ar.off))) return rc;   // problems + inputs
    if (br.off) HIP_TRY(hipMemcpyAsync(c->d_bound, c->h_bound, br.off, hipMemcpyHostToDevice, c->stream));
    c->uploaded = true;
    c->in_flight = true;
    return FX_OK;
}

int32_t fx_upload(FxContext *c, const FxProblem *prob) { return fx_upload_batch(c, 1, prob); }

// the device's answer to the one-launch step's sizing (one occupancy query per (CH, lds) of this process and device)
static int step_kernel_capacity(int device, int CH, size_t lds) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, size_t>, int> seen;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(device, CH, lds);
    auto it = seen.find(key);
    if (it == seen.end()) {
        int v = 0;
        if (fx_step_kernel_capacity(CH, lds, &v) != hipSuccess) { (void)hipGetLastError(); v = 0; }
        it = seen.emplace(key, v).first;
    }
    return it->second;
}

int32_t fx_evaluate(FxContext *c) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    if (!c->uploaded) return set_err(FX_ERR_NOT_READY, "fx_evaluate before fx_upload");
    if (c->timed_out) return set_err(FX_ERR_TIMEOUT, "an earlier wait on this context timed out: destroy it (its stream may never drain)");
    // (a planner's thread stays on its context's device from step to step: the device is set only where it is another one)
    int cur_device = -1;
    if (hipGetDevice(&cur_device) != hipSuccess || cur_device != c->device) HIP_TRY(hipSetDevice(c->device));
    if (c->probs_dirty || c->dirty_hi > c->dirty_lo) {
        // inputs rewritten by fx_update_state since the last evaluation: ONE copy of the front of the staging block (the
        // problems, then whatever changed behind them)
        const size_t lo = c->probs_dirty ? 0 : c->dirty_lo;
        const size_t hi = std::max(c->dirty_hi > c->dirty_lo ? c->dirty_hi : 0, c->probs_dirty ? sizeof(DevProblem) * (size_t)c->n_agents : 0);
        int rc = stage_range(c, lo, hi);
        if (rc) return rc;
        c->dirty_lo = (size_t)-1; c->dirty_hi = 0;
        c->probs_dirty = false;
    }
    const FxStepPlan &pl = c->plan;
    FxLaunchPlan &L = c->launch = fx_plan_launches(pl, c->force, c->package_enabled);
    // timing (every timing_every-th step): FX_TIMING_KERNEL attaches start/stop events to the evaluation kernel
    // itself (hipExtLaunchKernel), so its duration is the kernel's, not launch latency; FX_TIMING_STREAM brackets
    // with stream events instead (includes the dispatch gap before the kernel).  Events live in a ring and are
    // only read on request.
    const bool timed = c->timing != FX_TIMING_OFF && (c->n_steps % c->timing_every) == 0;
    c->n_steps++;
    const bool attached = timed && c->timing == FX_TIMING_KERNEL && L.eval_launched;
    FxContext::TimeSlot *ts = nullptr;
    if (timed) {
        ts = &c->ring[c->n_timed % FxContext::kTimeRing];
        ts->fetched = false;
        ts->eval_launched = L.eval_launched;
        ts->obst_timed = false;
    }
    hipEvent_t k0 = attached ? ts->e0 : nullptr, k1 = attached ? ts->e_eval : nullptr;
    if (timed && !attached) HIP_TRY(hipEventRecord(ts->e0, c->stream));
    c->seq++;
    double *winner = c->dev_winner ? c->dev_winner : (L.pkg ? c->d_winner_own : nullptr);
    double *host_pkg = L.pkg ? c->h_pkg.dev : nullptr;
    FuseArgs fuse{L.fused ? c->h_counters.dev : nullptr, c->seq, winner, (int32_t)((uint32_t)pl.K_max | (L.tail << 16))};
    // ---- the whole step in ONE launch (fx_step_kernel.h) where the upload qualifies and the device holds the launch at once ----
    if (L.try_step_kernel) {
        int cap[3] = {0, 0, 0};
        for (int q = 0; q < 3; q++)
            if (!c->force.step_kernel_CH || c->force.step_kernel_CH == FX_STEP_KERNEL_CHS[q])
                cap[q] = step_kernel_capacity(c->device, FX_STEP_KERNEL_CHS[q], fx_step_kernel_lds(pl, FX_STEP_KERNEL_CHS[q]));
        const FxStepKernelSize sz = fx_plan_step_kernel(pl, c->force, c->last_live, cap);
        if (sz.CH) {
            StepArgs sa{};
            sa.bar = c->d_bar; sa.bar_base = c->bar_base;
            sa.host_result = c->h_counters.dev; sa.seq = c->seq; sa.dev_winner = winner;
            sa.host_pkg = host_pkg; sa.pkg_stride = c->pkg_stride; sa.pkg_plane_rows = c->pkg_plane_rows;
            sa.walk_blocks = pl.max_blocks;
            HIP_TRY(fx_launch_step(c->d_probs, c->n_agents, sz.blocks, sz.lds, sz.CH, k0, k1, fuse, sa, c->stream));
            c->bar_base += (unsigned long long)sz.blocks * (unsigned long long)c->n_agents;
            fx_take_step_kernel(L, sz);
        }
    }
    if (L.eval_launched && !L.step_kernel) {
        if (pl.use_grid)
            HIP_TRY(fx_launch_eval_grid(c->d_probs, c->n_agents, pl.max_blocks, pl.block, pl.lds, pl.G, pl.any_bundle, pl.any_obst, pl.wpe,
                                        pl.wsplit, k0, k1, fuse, c->stream));
        else
            HIP_TRY(fx_launch_eval(c->d_probs, c->n_agents, pl.max_blocks, fx_generic_lds(pl.M_max, pl.S_max, pl.gen_rec_lds), pl.G,
                                   pl.any_bundle, pl.any_obst, pl.any_extra, pl.wpe, k0, k1, fuse, c->stream));
    }
    if (timed && !attached) HIP_TRY(hipEventRecord(ts->e_eval, c->stream));
    // one agent: the kernels of the split step take what their first loads need from their leading arguments (the host's copy of
    // the problem is the staged one: fx_update_state rewrites it and the staging above has copied it)
    const DevProblem *head = c->n_agents == 1 ? &c->h_probs[0] : nullptr;
    if (L.obstacle) {
        const bool t_obs = timed && c->timing == FX_TIMING_KERNEL;
        HIP_TRY(fx_launch_obstacle(c->d_probs, c->n_agents, pl.obs_blocks, L.obs_lds, pl.split_CH, t_obs ? ts->e_obs0 : nullptr,
                                   t_obs ? ts->e_obs1 : nullptr, c->stream, L.obs_wg, pl.obs_tiles, head));
        if (timed) ts->obst_timed = t_obs;
    }
    if (L.select)
        HIP_TRY(fx_launch_select(c->d_probs, c->n_agents, pl.C_max, c->h_counters.dev, c->seq, winner, host_pkg, c->pkg_stride,
                                 c->pkg_plane_rows, c->stream, head));
    if (L.package)
        HIP_TRY(fx_launch_package(c->d_probs, c->n_agents, winner, c->h_pkg.dev, c->pkg_stride, c->pkg_plane_rows, c->seq, c->stream));
    if (timed && !L.one_launch) HIP_TRY(hipEventRecord(ts->e_end, c->stream));
    if (timed) { ts->fused = L.one_launch; c->n_timed++; }
    c->timed_step = timed;
    c->evaluated = true;
    c->in_flight = true;
    return FX_OK;
}

int32_t fx_finish_batch(FxContext *c, FxResult *res) {
    if (!c || !res) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_finish: NULL argument");
    if (!c->evaluated) return set_err(FX_ERR_NOT_READY, "fx_finish before fx_evaluate");
    // wait for the sequence words the selection kernel publishes (bounded in TIME: fx_set_timeout_ms)
    for (int a = 0; a < c->n_agents; a++) {
        // with a winner package the last word to arrive is the package's (its kernel runs behind the selection)
        const volatile unsigned long long *sq = c->launch.pkg
            ? reinterpret_cast<const unsigned long long *>(c->h_pkg + (size_t)a * c->pkg_stride + c->pkg_stride - 1)
            : c->h_counters + (size_t)a * (FX_CNT_COUNT + 1) + FX_CNT_COUNT;
        int rc = wait_seq(c, sq, c->seq);
        if (rc) return rc;
    }
    c->in_flight = false;
    // device time of this step: only if its events have already completed (a timed step never waits for them here;
    // fx_last_kernel_ms / fx_read_kernel_times do)
    double step_ms = -1.0;
    if (c->timed_step) {
        FxContext::TimeSlot &t = c->ring[(c->n_timed - 1) % FxContext::kTimeRing];
        if (t.fetched || hipEventQuery(t.fused ? t.e_eval : t.e_end) == hipSuccess) {
            int rc = fetch_slot(c, t);
            if (rc) return rc;
            step_ms = t.step_ms;
        } else (void)hipGetLastError();  // hipErrorNotReady is not an error
    }
    for (int a = 0; a < c->n_agents; a++) {
        const unsigned long long *cn = c->h_counters + (size_t)a * (FX_CNT_COUNT + 1);
        FxResult &r = res[a];
        memset(&r, 0, sizeof(r));
        r.n_candidates = c->slots[a].C;
        r.n_returned = (int64_t)cn[FX_CNT_RETURNED];
        r.n_feasible = (int64_t)cn[FX_CNT_FEASIBLE];
        r.n_infeasible = r.n_returned - r.n_feasible;
        for (int k = 0; k < FX_NUM_REASONS; k++) r.reason_hist[k] = (int64_t)cn[FX_CNT_HIST0 + k];
        r.best_index = cn[FX_CNT_BEST_IDX] == ~0ULL ? -1 : (int64_t)cn[FX_CNT_BEST_IDX];
        double bc;
        memcpy(&bc, &cn[FX_CNT_BEST_COST], sizeof(bc));
        r.best_cost = r.best_index < 0 ? 0.0 : bc;
        r.n_collisions = (int64_t)cn[FX_CNT_COLLISIONS];
        r.feasible_percentage = r.n_returned ? 100.0 * ((double)r.n_feasible / (double)r.n_returned) : 0.0;
        r.kernel_ms = step_ms;
        // (costed candidates of the step: the feasible ones, with draw_traj_set everything returned -- sizes the next one-launch step)
        const int64_t live = (c->slots[a].mode & FX_MODE_DRAW_TRAJ_SET) ? r.n_returned : r.n_feasible;
        c->last_live = a == 0 ? live : std::max(c->last_live, live);
    }
    return FX_OK;
}

int32_t fx_finish(FxContext *c, FxResult *res) { return fx_finish_batch(c, res); }

int32_t fx_step(FxContext *c, FxResult *res) {
    const int rc = fx_evaluate(c);
    return rc ? rc : fx_finish_batch(c, res);
}

// Per-step state of one agent of the uploaded batch (header: fxplan.h).
int32_t fx_update_state(FxContext *c, int32_t agent, const FxStateUpdate *u) {
    if (!c || !u) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_update_state: NULL argument");
    if (!c->uploaded) return set_err(FX_ERR_NOT_READY, "fx_update_state before fx_upload");
    if (agent < 0 || agent >= c->n_agents) return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d out of range", agent);
    if (c->in_flight) {  // a copy out of the staging block may still be running: let it land before rewriting its source
        HIP_TRY(hipSetDevice(c->device));
        FX_TRY(fx_drain(c));
        c->in_flight = false;
    }
    FxAgentSlot &sl = c->slots[agent];
    DevProblem &d = c->h_probs[agent];
    // every argument is checked BEFORE anything is rewritten: an update that is refused leaves the context as it was
    if ((u->t_samp || u->v_samp || u->d_samp) && sl.off_t == (size_t)-1)
        return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d was uploaded with a sampling matrix: upload again", agent);
    if ((u->obs_pos || u->obs_cov_inv || u->obs_npred || u->obs_hull || u->obs_nhull) && sl.K <= 0)
        return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d was uploaded without obstacles: upload again", agent);
    if ((u->obs_hull || u->obs_nhull) && !sl.have_hull)
        return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d was uploaded without obstacle hulls: upload again", agent);
    if ((u->t_samp && u->nT && u->nT != sl.nT) || (u->v_samp && u->nV && u->nV != sl.nV) || (u->d_samp && u->nD && u->nD != sl.nD))
        return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d: sampling arrays of %d x %d x %d values, uploaded %d x %d x %d: upload again", agent,
                       u->nT, u->nV, u->nD, sl.nT, sl.nV, sl.nD);
    if ((u->obs_pos || u->obs_cov_inv || u->obs_npred || u->obs_hull || u->obs_nhull) && ((u->K && u->K != sl.K) || (u->P && u->P != sl.P)))
        return set_err(FX_ERR_INVALID_ARGUMENT, "agent %d: obstacle arrays for K = %d, P = %d, uploaded K = %d, P = %d: upload again", agent,
                       u->K, u->P, sl.K, sl.P);
    auto touch = [&](size_t off, size_t bytes) {
        c->dirty_lo = std::min(c->dirty_lo, off);
        c->dirty_hi = std::max(c->dirty_hi, off + bytes);
    };
    bool origin_moved = false;
    if (u->x0_lon) {
        origin_moved = d.x0_lon[0] != u->x0_lon[0];
        memcpy(d.x0_lon, u->x0_lon, sizeof(d.x0_lon));
    }
    if (u->x0_lat) memcpy(d.x0_lat, u->x0_lat, sizeof(d.x0_lat));
    if (u->x0_orientation == u->x0_orientation) d.x0_orientation = u->x0_orientation;
    if (u->v_des == u->v_des) d.v_des = u->v_des;
    if (u->low_vel_mode >= 0) d.low_vel_mode = u->low_vel_mode;
    if (u->t_samp || u->v_samp || u->d_samp) {
        if (u->t_samp) { memcpy(c->h_in + sl.off_t, u->t_samp, sizeof(double) * sl.nT); touch(sl.off_t, sizeof(double) * sl.nT); }
        if (u->v_samp) { memcpy(c->h_in + sl.off_v, u->v_samp, sizeof(double) * sl.nV); touch(sl.off_v, sizeof(double) * sl.nV); }
        if (u->d_samp) { memcpy(c->h_in + sl.off_d, u->d_samp, sizeof(double) * sl.nD); touch(sl.off_d, sizeof(double) * sl.nD); }
    }
    const bool new_obs = u->obs_pos || u->obs_cov_inv || u->obs_npred || u->obs_hull || u->obs_nhull;
    if (new_obs || (origin_moved && sl.K > 0)) {
        const int K = sl.K, P = sl.P, S = sl.S;
        double *pos = reinterpret_cast<double *>(c->h_in + sl.off_pos), *cov = reinterpret_cast<double *>(c->h_in + sl.off_cov);
        int32_t *npred = reinterpret_cast<int32_t *>(c->h_in + sl.off_npred);
        if (u->obs_pos) memcpy(pos, u->obs_pos, sizeof(double) * 2 * K * P);
        if (u->obs_cov_inv) memcpy(cov, u->obs_cov_inv, sizeof(double) * 4 * K * P);
        if (u->obs_npred) memcpy(npred, u->obs_npred, sizeof(int32_t) * K);
        double *hull = nullptr;
        int32_t *nhull = nullptr;
        if (sl.have_hull) {
            hull = reinterpret_cast<double *>(c->h_in + sl.off_hull);
            nhull = reinterpret_cast<int32_t *>(c->h_in + sl.off_nhull);
            if (u->obs_hull) memcpy(hull, u->obs_hull, sizeof(double) * 6 * K * (P - 1));
            if (u->obs_nhull) memcpy(nhull, u->obs_nhull, sizeof(int32_t) * K);
        }
        hot_origin_of(reinterpret_cast<const double *>(c->h_in + sl.off_ref), sl.M, d.x0_lon[0], d.hot_origin);
        d.hot_gap_margin = pack_obstacle_tables(S, K, P, pos, cov, npred, hull, nhull, sl.have_hull, d.hot_origin[0], d.hot_origin[1],
                                                reinterpret_cast<double *>(c->h_in + sl.off_rec),
                                                reinterpret_cast<unsigned long long *>(c->h_in + sl.off_pm),
                                                reinterpret_cast<unsigned long long *>(c->h_in + sl.off_hm),
                                                reinterpret_cast<double *>(c->h_in + sl.off_hot));
        // The walk reads the packed tables.  The raw predictions have ONE reader on the device, in the grid and the generic kernel
        // alike: with more than one lane per candidate and the obstacle stage inside the walk, a lane part that starts behind the
        // step at which its candidate left the projection domain re-sums its prediction cost from them (fx_eval_kernel.h,
        // finish_candidate).  They are staged with the tables when the update brought new ones and the plan has that reader.
        const bool raw_read = new_obs && c->plan.G > 1 && !c->plan.split;
        touch(sl.off_rec, (raw_read ? sl.raw_end : sl.dyn_end) - sl.off_rec);
    }
    c->probs_dirty = true;
    return FX_OK;
}

int32_t fx_update_step(FxContext *c, const FxStateUpdate *u, FxResult *res) {
    int rc = fx_update_state(c, 0, u);
    if (rc) return rc;
    return fx_step(c, res);
}

// ---- winner package (header: fxplan.h) ----
int32_t fx_set_package(FxContext *c, int32_t enabled) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "context is NULL");
    c->package_enabled = enabled != 0;
    return FX_OK;
}

int32_t fx_read_package(FxContext *c, int32_t agent, double yaw_rate0, FxPackage *pkg, double *block) {
    int rc = check_agent(c, agent);
    if (rc) return rc;
    if (!pkg) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_read_package: NULL argument");
    if (!c->launch.pkg) return set_err(FX_ERR_NOT_READY, "the last step ran without a winner package (fx_set_package, FX_MODE_WRITE_BUNDLE)");
    if (c->in_flight) {  // fx_finish has not been called for this step: wait for the package word here
        rc = wait_seq(c, reinterpret_cast<const unsigned long long *>(c->h_pkg + (size_t)agent * c->pkg_stride + c->pkg_stride - 1), c->seq);
        if (rc) return rc;
    }
    const FxAgentSlot &sl = c->slots[agent];
    const DevProblem &d = c->h_probs[agent];
    const double *src = c->h_pkg + (size_t)agent * c->pkg_stride, *tail = src + c->pkg_plane_rows;
    const int S = sl.S;
    memset(pkg, 0, sizeof(*pkg));
    pkg->S = S;
    pkg->n_cost = sl.n_cost;
    pkg->index = -1;
    pkg->found = tail[16 + FX_NUM_COSTS] != 0.0;
    if (!pkg->found) return FX_OK;
    memcpy(pkg->coeff_lon, tail, sizeof(double) * 6);
    memcpy(pkg->coeff_lat, tail + 6, sizeof(double) * 6);
    memcpy(pkg->raw_costs, tail + 12, sizeof(double) * FX_NUM_COSTS);
    pkg->cost = tail[12 + FX_NUM_COSTS];
    pkg->traj_len = (int32_t)tail[13 + FX_NUM_COSTS];
    pkg->flags = (uint32_t)tail[14 + FX_NUM_COSTS];
    pkg->index = (int64_t)tail[15 + FX_NUM_COSTS];
    pkg->tau_lat = tail[17 + FX_NUM_COSTS];
    if (!block) return FX_OK;
    memcpy(block, src, sizeof(double) * FX_NUM_PLANES * S);
    fx_package_derive(d, S, yaw_rate0, block);
    return FX_OK;
}

int32_t fx_plan_and_package(FxContext *c, const FxStateUpdate *upd, double yaw_rate0, FxResult *res, FxPackage *pkg, double *block) {
    if (!c || !res || !pkg) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_and_package: NULL argument");
    int rc;
#ifdef FX_HOST_PROBE   // probe builds: where the host side of a planner step goes (tools/probe_build)
    static double acc[4]; static int n_acc;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
#endif
    if (upd && (rc = fx_update_state(c, 0, upd))) return rc;
#ifdef FX_HOST_PROBE
    const double t1 = now();
#endif
    const bool was = c->package_enabled;
    c->package_enabled = true;
    rc = fx_evaluate(c);
    c->package_enabled = was;
    if (rc) return rc;
#ifdef FX_HOST_PROBE
    const double t2 = now();
#endif
    if ((rc = fx_finish_batch(c, res))) return rc;
#ifdef FX_HOST_PROBE
    const double t3 = now();
    rc = fx_read_package(c, 0, yaw_rate0, pkg, block);
    const double t4 = now();
    acc[0] += t1 - t0; acc[1] += t2 - t1; acc[2] += t3 - t2; acc[3] += t4 - t3;
    if (++n_acc == 200) {
        fprintf(stderr, "fx_plan_and_package: update_state %.1f us, evaluate (launches) %.1f us, finish (wait) %.1f us, read_package %.1f us\n",
                acc[0] / n_acc, acc[1] / n_acc, acc[2] / n_acc, acc[3] / n_acc);
        acc[0] = acc[1] = acc[2] = acc[3] = 0; n_acc = 0;
    }
    return rc;
#else
    return fx_read_package(c, 0, yaw_rate0, pkg, block);
#endif
}

int32_t fx_plan_batch_begin(FxContext *c, int32_t n_agents, const FxStateUpdate *const *upd) {
    if (!c) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_batch_begin: NULL argument");
    if (!c->uploaded) return set_err(FX_ERR_NOT_READY, "fx_plan_batch_begin before fx_upload");
    if (n_agents != c->n_agents)
        return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_batch_begin: %d agents, the uploaded batch has %d", n_agents, c->n_agents);
    int rc;
    if (upd)
        for (int a = 0; a < n_agents; a++)
            if (upd[a] && (rc = fx_update_state(c, a, upd[a]))) return rc;
    const bool was = c->package_enabled;
    c->package_enabled = true;
    rc = fx_evaluate(c);
    c->package_enabled = was;
    return rc;
}

int32_t fx_plan_batch_end(FxContext *c, int32_t n_agents, const double *yaw_rate0, FxResult *res, FxPackage *pkg, double *const *blocks) {
    if (!c || !res || !pkg) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_batch_end: NULL argument");
    if (n_agents != c->n_agents)
        return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_batch_end: %d agents, the uploaded batch has %d", n_agents, c->n_agents);
    int rc;
    if ((rc = fx_finish_batch(c, res))) return rc;
    for (int a = 0; a < n_agents; a++)
        if ((rc = fx_read_package(c, a, yaw_rate0 ? yaw_rate0[a] : 0.0, pkg + a, blocks ? blocks[a] : nullptr))) return rc;
    return FX_OK;
}

int32_t fx_plan_batch_packaged(FxContext *c, int32_t n_agents, const FxStateUpdate *const *upd, const double *yaw_rate0, FxResult *res,
                               FxPackage *pkg, double *const *blocks) {
    if (!c || !res || !pkg) return set_err(FX_ERR_INVALID_ARGUMENT, "fx_plan_batch_packaged: NULL argument");
#ifdef FX_HOST_PROBE   // probe builds: where the host side of a batched planner step goes (tools/probe_build)
    static double acc[2]; static int n_acc;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
#endif
    int rc = fx_plan_batch_begin(c, n_agents, upd);
    if (rc) return rc;
#ifdef FX_HOST_PROBE
    const double t1 = now();
#endif
    rc = fx_plan_batch_end(c, n_agents, yaw_rate0, res, pkg, blocks);
#ifdef FX_HOST_PROBE
    acc[0] += t1 - t0; acc[1] += now() - t1;
    if (++n_acc == 20) {
        fprintf(stderr, "fx_plan_batch_packaged: begin (state updates, launches) %.1f us, end (wait, packages) %.1f us\n", acc[0] / n_acc,
                acc[1] / n_acc);
        acc[0] = acc[1] = 0; n_acc = 0;
    }
#endif
    return rc;
}

int32_t fx_plan_step(FxContext *c, const FxProblem *prob, FxResult *res) {
    int rc = fx_upload(c, prob);
    if (rc) return rc;
    if ((rc = fx_evaluate(c))) return rc;
    return fx_finish(c, res);
}

}  // extern "C"
