// fx_eval_list_kernel.h -- the list form of the generic evaluation kernel (fx_eval_kernel.h at one lane per candidate):
// re-walks a caller's list of candidates of the last plan step and stores their bundle rows, coefficients, cost map, cost,
// flags and boundary steps into a compact structure-of-arrays block, the agent's "sparse set" (fx_materialise_candidates_agent;
// DESIGN.md section 14).
//
// Lane `pos` of the launch walks candidate ids[pos] -- the candidate's parameters come from ids[pos] + g_base, every output goes
// to column pos of the problem's arrays.  The problem is a CLONE of the agent's DevProblem whose outputs (planes, coeffs,
// traj_len, costmap, cost, flags, bound_step) and selection scratch (counters, part_cost, part_idx) address the sparse block,
// with C = n, ld = n rounded up to 64, the bundle and the cost map on, FX_MODE_INT_DEFER_OBST off: nothing of the step is
// written.  The arithmetic is the step's own -- lon_coeffs, lon_goal_span, lat_quintic, traj_len_of, make_lon_row, lat_at,
// fill_step_const, walk_step with the obstacle stage fused in and finish_candidate are the functions the generic kernel calls
// (fx_walk.h, fx_eval_kernel.h) -- so a row equals the row the generic kernel stores for that candidate bit for bit.  Table
// staging, candidate parameters, coefficient store, windowed terms and the accumulators' hand-over are still written out here
// as in fx_eval_kernel.h: made a shared function, each of them changed the generic kernels' instruction text.
//
// The launch passes no fused selection (FuseArgs.host_result == nullptr): finish_candidate stores the outputs, adds to the
// clone's own counters, writes the workgroup's arg-min partial into the clone's scratch and returns.  No tail, no ticket, no
// wait loop, no published word: like the gather kernel it cannot hang.
//
// grid = ceil(n / 256), block = 256, dynamic LDS as fx_eval_kernel: M * 64 B knots + FX_TP * S * 8 B time table + M arc lengths.
#pragma once

#include "fx_eval_kernel.h"

//   OBST  : obstacles present and / or the road-boundary stage (prediction cost, OBB collision walk, boundary walk)
//   EXTRA : windowed cost terms active (Simpson integrals, distance_to_obstacles, lane_center_offset)
template <bool OBST, bool EXTRA>
__global__ __launch_bounds__(FX_BLOCK, 2) void fx_eval_list_kernel(const DevProblem *__restrict__ prob, const int64_t *__restrict__ ids) {
    using namespace fxk;
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];  // [M][8] knots, the [S][FX_TP] time table, [M] arc lengths
    __shared__ double red_cost[FX_BLOCK / 64];
    __shared__ long long red_idx[FX_BLOCK / 64];
    __shared__ unsigned int red_cnt[2 + FX_NUM_REASONS + 1];
    __shared__ int32_t sh_cost_id[FX_NUM_COSTS];
    __shared__ double sh_cost_w[FX_NUM_COSTS];

    const DevProblem &Pg = prob[0];
    const ProblemRegs P = ProblemRegs::load(Pg, sh_cost_id, sh_cost_w);
    const int tid = threadIdx.x;
    const int64_t n = P.C;   // (the clone's C is the length of the list)
    if ((int64_t)blockIdx.x * FX_BLOCK >= n) return;
    const int64_t pos_raw = (int64_t)blockIdx.x * FX_BLOCK + tid;
    const bool active = pos_raw < n;
    const int64_t g = active ? pos_raw : n - 1;            // output column
    const int64_t gg = as_global(ids)[g] + P.g_base;       // global candidate index: the sampling row / grid point

    const int M = P.M, S = P.S;
    double *__restrict__ rpos = lds_dyn + (size_t)M * FX_REF_FIELDS + (size_t)FX_TP * S;
    {
        const FX_GLOBAL double *__restrict__ src = as_global(P.ref);
        for (int i = tid; i < M * FX_REF_FIELDS; i += FX_BLOCK) {
            const double v = src[i];
            lds_dyn[i] = v;
            if ((i & (FX_REF_FIELDS - 1)) == 0) rpos[i / FX_REF_FIELDS] = v;
        }
        const FX_GLOBAL double *__restrict__ tsrc = as_global(P.tpow);
        for (int i = tid; i < S; i += FX_BLOCK)
            fill_time_row(lds_dyn + M * FX_REF_FIELDS + i * FX_TP, tsrc[i], tsrc[S + i], tsrc[2 * S + i], tsrc[3 * S + i], tsrc[4 * S + i]);
        if (tid < P.n_cost) { sh_cost_id[tid] = Pg.cost_id[tid]; sh_cost_w[tid] = Pg.cost_w[tid]; }
    }
    if (tid < 2 + FX_NUM_REASONS) red_cnt[tid] = 0;
    __syncthreads();
    const Knot *__restrict__ knots = reinterpret_cast<const Knot *>(lds_dyn);
    const double *__restrict__ tp = lds_dyn + M * FX_REF_FIELDS;

    const double dt = P.dt;
    const bool low_vel = P.low_vel_mode != 0;
    const bool D = (P.mode & FX_MODE_DRAW_TRAJ_SET) != 0;
    const bool dbg = D || (P.mode & FX_MODE_KINEMATIC_DEBUG) != 0;
    const bool do_collision = OBST && (P.mode & FX_MODE_COLLISION) != 0;
    const bool bundle = (P.mode & FX_MODE_WRITE_BUNDLE) != 0;   // (the host sets it in the clone)
    const double a_max = P.veh.a_max;
    const int64_t ld = P.ld;

    // ---- candidate parameters: fx_eval_kernel.h, the same expressions ----
    double T, s0, ss0, sss0, v1, a1, d0, dd0, ddd0, d1, dd1, ddd1;
    if (P.has_matrix) {
        const FX_GLOBAL double *__restrict__ r = as_global(P.matrix) + 13 * gg;
        T = r[1] - r[0];
        s0 = r[2]; ss0 = r[3]; sss0 = r[4]; v1 = r[5]; a1 = r[6];
        d0 = r[7]; dd0 = r[8]; ddd0 = r[9]; d1 = r[10]; dd1 = r[11]; ddd1 = r[12];
    } else {
        const int nD = P.nD, nV = P.nV;
        const int64_t q = gg / nD;
        const int id = (int)(gg - q * nD);
        const int it = (int)(q / nV);
        const int iv = (int)(q - (int64_t)it * nV);
        T = as_global(P.t_samp)[it];
        v1 = as_global(P.v_samp)[iv];
        d1 = as_global(P.d_samp)[id];
        s0 = P.x0_lon[0]; ss0 = P.x0_lon[1]; sss0 = P.x0_lon[2];
        d0 = P.x0_lat[0]; dd0 = P.x0_lat[1]; ddd0 = P.x0_lat[2];
        a1 = 0.0; dd1 = 0.0; ddd1 = 0.0;
    }
    double cl0 = s0, cl1 = ss0, cl2 = .5 * sss0, cl3, cl4, cl5;
    lon_coeffs(P.has_matrix ? FX_LON_VELOCITY_KEEPING : P.lon_mode, s0, ss0, sss0, T, v1, a1, cl3, cl4, cl5);
    double tau = T;
    if (low_vel) tau = lon_goal_span(T, s0, cl0, cl1, cl2, cl3, cl4, cl5);
    LatPoly L;
    lat_quintic(L, tau, d0, dd0, ddd0, d1, dd1, ddd1);
    const int traj_len = traj_len_of(T, dt, S);

    if (bundle && active) {
        FX_GLOBAL double *__restrict__ co = as_global(P.coeffs) + g;
        const double cv[FX_COEFF_ROWS] = {cl0, cl1, cl2, cl3, cl4, cl5, L.c0, L.c1, L.c2, L.c3, L.c4, L.c5, tau};
#pragma unroll
        for (int q = 0; q < FX_COEFF_ROWS; q++) st_out(co + q * ld, cv[q], false);
        st_out(as_global(P.traj_len) + g, (int32_t)traj_len, false);
    }

    const double rp_first = knots[0].pos, rp_last = knots[M - 1].pos;
    const double guess_scale = fdiv((double)(M - 1), rp_last - rp_first);
    const bool want_trig = OBST && ((do_collision && P.K > 0) || ((P.mode & FX_MODE_ROAD_BOUNDARY) && P.n_bound > 0));
    auto row_at = [&](int i) {
        return make_lon_row(i, S, M, dt, a_max, cl0, cl1, cl2, cl3, cl4, cl5, traj_len, tp, rp_first, rp_last, guess_scale,
                            want_trig, [&](int k) { return knots[k]; }, [&](int k) { return rpos[k]; },
                            (P.mode & FX_MODE_PROJ_PSEUDO_NORMAL) != 0);
    };
    auto lat_eval = [&](int i, double u_lowvel, double &d, double &dv, double &da) { lat_at(L, low_vel, tp, i, u_lowvel, d, dv, da); };
    double d_ext, dv_u, da_u;
    {
        const LonRow rl = row_at(traj_len - 1);
        lat_eval(traj_len - 1, rl.u1, d_ext, dv_u, da_u);
    }

    StepConst K;
    fill_step_const<OBST>(K, P);
    K.low_vel = low_vel; K.dbg = dbg; K.do_collision = do_collision; K.store_wt = (P.mode & FX_MODE_INT_STORE_WT) != 0;
    K.atan_k = nullptr;
    const BoundView Bv{as_global(P.bound_piece), as_global(P.bound_bin), as_global(P.bound_item)};
    const FX_GLOBAL double *__restrict__ obs_rec = as_global(P.obs_rec);
    const FX_GLOBAL unsigned long long *__restrict__ obs_pmask = as_global(P.obs_pmask);
    const FX_GLOBAL unsigned long long *__restrict__ obs_hmask = as_global(P.obs_hmask);

    StepCarry Cy;
    Cy.reset(P.x0_orientation);
    StepAcc A;
    A.reset();
    StepOut O;
    Simpson sim_acc, sim_jerk, sim_orient, sim_path;
    double a_prev = 0.0, thcl_prev = 0.0, dto = 0.0;
    if (EXTRA) { sim_acc.init(); sim_jerk.init(); sim_orient.init(); sim_path.init(); }
    const int n_dto = EXTRA ? P.n_dto : 0;
    const FX_GLOBAL double *__restrict__ dto_pos = as_global(P.dto_pos);
    bool lane_on = false;
    if (EXTRA)
        for (int q = 0; q < P.n_cost; q++) lane_on |= P.cost_id[q] == FX_COST_LANE_CENTER_OFFSET;
    double lane_off = 0.0;
    FX_GLOBAL double *__restrict__ planes = as_global(P.planes);
    const int64_t ps = (int64_t)S * ld;

#pragma unroll 1
    for (int i = 0; i < S; i++) {
        const LonRow r = row_at(i);
        walk_step<OBST, true>(K, r, L, tp, i, traj_len, d_ext, true, bundle && active, planes + (int64_t)i * ld + g, 0u, ps, Cy, A, O,
                              obs_rec, obs_pmask, obs_hmask, Bv, nullptr, -1, false, false);
        if (EXTRA) {   // the windowed terms: fx_eval_kernel.h, partial_cost_functions.py
            sim_acc.push(O.a * O.a, S);
            sim_path.push(O.v, S);
            if (i > 0) {
                const double j = (O.a - a_prev) / dt;
                const double w = (O.th_cl - thcl_prev) / dt;
                sim_jerk.push(j * j, S - 1);
                sim_orient.push(w * w, S - 1);
            }
            a_prev = O.a;
            thcl_prev = O.th_cl;
            for (int o = 0; o < n_dto; o++) {
                const double ex = O.x - dto_pos[2 * o], ey = O.y - dto_pos[2 * o + 1];
                const double dist = sqrt(ex * ex + ey * ey);
                dto += 1.0 / (dist * dist);
            }
            if (lane_on) lane_off += lane_center_distance(P, O.x, O.y);
        }
    }

    WalkResult W;
    W.neg = A.neg; W.acc_viol = A.acc_viol; W.collided = A.collided;
    W.step_reasons = A.step_reasons; W.first_key = A.first_key; W.fail_step = A.fail_step; W.bound_step = A.bound_step;
    W.sum_abs_d = A.sum_abs_d; W.sum_voff = A.sum_voff; W.pred = A.pred; W.dto = dto; W.lane_off = lane_off; W.d_end = A.d_end; W.v_end = A.v_end;
    W.set_poly(cl3, cl4, cl5, L);
    if (EXTRA) { W.sim_acc = sim_acc; W.sim_jerk = sim_jerk; W.sim_orient = sim_orient; W.sim_path = sim_path; }
    const FuseArgs no_fuse{nullptr, 0ULL, nullptr, 0};   // no fused selection, no tail: the outputs and the clone's own scratch only
    finish_candidate<1, true, OBST, EXTRA>(P, Pg, W, g, active, 0, 0, S, bundle, do_collision, dbg, D, red_cost, red_idx, red_cnt, no_fuse);
}

// ---------------------------------------------------------------------------------------------------
// The list kernel over a TABLE of rows, on split lanes (fx_materialise_candidates_batch, fx_set_materialise_lanes; DESIGN.md
// section 22).  blockIdx.y selects a row -- a listed agent's clone and its list -- and within the row the kernel is
// fx_eval_kernel<G, true, OBST, EXTRA>'s decomposition with the candidate's index read from the list: G adjacent lanes per
// candidate and 256 / G candidates per workgroup, part = tid & (G - 1), chunks of ceil(S / G) steps, the carry-in step of parts
// > 0 (at one step per lane the left lane's hand-over, walk_step's `neigh`), the re-run of the horizon extension, the standstill
// heading scan, and finish_candidate's shuffle combine.  Every function is the one the generic kernel calls, so a row equals the
// row the generic kernel forced to G lanes stores for that candidate bit for bit.  The step's obstacle records come from global
// memory (the clone has FX_MODE_INT_REC_LDS off): the same values the generic kernel stages into LDS.
//
// A clone's n_blocks is ceil(C / (256 / G)); a workgroup whose first candidate lies beyond its row's count returns before any
// barrier.  No fused selection is passed: FX_TAIL_IN_KERNEL compiles the tail in from G = 4 on, and without a result block it
// stays off -- no ticket, no wait loop, no published word.
//
// grid = (ceil(max C / (256 / G)), rows), block = 256, dynamic LDS as fx_eval_list_kernel for the largest row of the launch.
// ---------------------------------------------------------------------------------------------------
template <int G, bool OBST, bool EXTRA>
// (one wave per SIMD where the obstacle stage or the windowed terms are in: at two the one-lane forms spill -- 20 to 244 bytes of
// scratch per lane -- and a list is a handful of workgroups on an idle chip, where the second wave buys nothing)
__global__ __launch_bounds__(FX_BLOCK, (OBST || EXTRA) ? 1 : 2) void fx_eval_list_rows_kernel(const EvalListRow *__restrict__ rows) {
    using namespace fxk;
    static_assert(!EXTRA || G == 1, "windowed costs need the whole horizon in one lane");
    static_assert(G == 1 || G == 8 || G == 32, "the list kernel's lane splits");
    constexpr int CPB = FX_BLOCK / G;  // candidates per workgroup
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];  // [M][8] knots, the [S][FX_TP] time table, [M] arc lengths
    __shared__ double red_cost[FX_BLOCK / 64];
    __shared__ long long red_idx[FX_BLOCK / 64];
    __shared__ unsigned int red_cnt[2 + FX_NUM_REASONS + 1];
    __shared__ int32_t sh_cost_id[FX_NUM_COSTS];
    __shared__ double sh_cost_w[FX_NUM_COSTS];

    const EvalListRow row = rows[blockIdx.y];
    const DevProblem &Pg = row.clone[0];
    const ProblemRegs P = ProblemRegs::load(Pg, sh_cost_id, sh_cost_w);
    const int tid = threadIdx.x;
    const int64_t n = P.C;   // (the clone's C is the length of the list)
    if ((int64_t)blockIdx.x * CPB >= n) return;  // whole workgroup beyond this row's list
    const int part = G == 1 ? 0 : (tid & (G - 1));
    const int64_t pos_raw = (int64_t)blockIdx.x * CPB + (G == 1 ? tid : tid / G);
    const bool active = pos_raw < n;
    const int64_t g = active ? pos_raw : n - 1;                // output column
    const int64_t gg = as_global(row.ids)[g] + P.g_base;       // global candidate index: the sampling row / grid point

    const int M = P.M, S = P.S;
    double *__restrict__ rpos = lds_dyn + (size_t)M * FX_REF_FIELDS + (size_t)FX_TP * S;
    {
        const FX_GLOBAL double *__restrict__ src = as_global(P.ref);
        for (int i = tid; i < M * FX_REF_FIELDS; i += FX_BLOCK) {
            const double v = src[i];
            lds_dyn[i] = v;
            if ((i & (FX_REF_FIELDS - 1)) == 0) rpos[i / FX_REF_FIELDS] = v;
        }
        const FX_GLOBAL double *__restrict__ tsrc = as_global(P.tpow);
        for (int i = tid; i < S; i += FX_BLOCK)
            fill_time_row(lds_dyn + M * FX_REF_FIELDS + i * FX_TP, tsrc[i], tsrc[S + i], tsrc[2 * S + i], tsrc[3 * S + i], tsrc[4 * S + i]);
        if (tid < P.n_cost) { sh_cost_id[tid] = Pg.cost_id[tid]; sh_cost_w[tid] = Pg.cost_w[tid]; }
    }
    if (tid < 2 + FX_NUM_REASONS) red_cnt[tid] = 0;
    __syncthreads();
    const Knot *__restrict__ knots = reinterpret_cast<const Knot *>(lds_dyn);
    const double *__restrict__ tp = lds_dyn + M * FX_REF_FIELDS;

    const double dt = P.dt;
    const bool low_vel = P.low_vel_mode != 0;
    const bool D = (P.mode & FX_MODE_DRAW_TRAJ_SET) != 0;
    const bool dbg = D || (P.mode & FX_MODE_KINEMATIC_DEBUG) != 0;
    const bool do_collision = OBST && (P.mode & FX_MODE_COLLISION) != 0;
    const bool bundle = (P.mode & FX_MODE_WRITE_BUNDLE) != 0;   // (the host sets it in the clone)
    const double a_max = P.veh.a_max;
    const int64_t ld = P.ld;

    // ---- candidate parameters: fx_eval_kernel.h, the same expressions ----
    double T, s0, ss0, sss0, v1, a1, d0, dd0, ddd0, d1, dd1, ddd1;
    if (P.has_matrix) {
        const FX_GLOBAL double *__restrict__ r = as_global(P.matrix) + 13 * gg;
        T = r[1] - r[0];
        s0 = r[2]; ss0 = r[3]; sss0 = r[4]; v1 = r[5]; a1 = r[6];
        d0 = r[7]; dd0 = r[8]; ddd0 = r[9]; d1 = r[10]; dd1 = r[11]; ddd1 = r[12];
    } else {
        const int nD = P.nD, nV = P.nV;
        const int64_t q = gg / nD;
        const int id = (int)(gg - q * nD);
        const int it = (int)(q / nV);
        const int iv = (int)(q - (int64_t)it * nV);
        T = as_global(P.t_samp)[it];
        v1 = as_global(P.v_samp)[iv];
        d1 = as_global(P.d_samp)[id];
        s0 = P.x0_lon[0]; ss0 = P.x0_lon[1]; sss0 = P.x0_lon[2];
        d0 = P.x0_lat[0]; dd0 = P.x0_lat[1]; ddd0 = P.x0_lat[2];
        a1 = 0.0; dd1 = 0.0; ddd1 = 0.0;
    }
    double cl0 = s0, cl1 = ss0, cl2 = .5 * sss0, cl3, cl4, cl5;
    lon_coeffs(P.has_matrix ? FX_LON_VELOCITY_KEEPING : P.lon_mode, s0, ss0, sss0, T, v1, a1, cl3, cl4, cl5);
    double tau = T;
    if (low_vel) tau = lon_goal_span(T, s0, cl0, cl1, cl2, cl3, cl4, cl5);
    LatPoly L;
    lat_quintic(L, tau, d0, dd0, ddd0, d1, dd1, ddd1);
    const int traj_len = traj_len_of(T, dt, S);

    if (bundle && active && part == 0) {
        FX_GLOBAL double *__restrict__ co = as_global(P.coeffs) + g;
        const double cv[FX_COEFF_ROWS] = {cl0, cl1, cl2, cl3, cl4, cl5, L.c0, L.c1, L.c2, L.c3, L.c4, L.c5, tau};
#pragma unroll
        for (int q = 0; q < FX_COEFF_ROWS; q++) st_out(co + q * ld, cv[q], false);
        st_out(as_global(P.traj_len) + g, (int32_t)traj_len, false);
    }

    const double rp_first = knots[0].pos, rp_last = knots[M - 1].pos;
    const double guess_scale = fdiv((double)(M - 1), rp_last - rp_first);
    const bool want_trig = OBST && ((do_collision && P.K > 0) || ((P.mode & FX_MODE_ROAD_BOUNDARY) && P.n_bound > 0));
    auto row_at = [&](int i) {
        return make_lon_row(i, S, M, dt, a_max, cl0, cl1, cl2, cl3, cl4, cl5, traj_len, tp, rp_first, rp_last, guess_scale,
                            want_trig, [&](int k) { return knots[k]; }, [&](int k) { return rpos[k]; },
                            (P.mode & FX_MODE_PROJ_PSEUDO_NORMAL) != 0);
    };
    auto lat_eval = [&](int i, double u_lowvel, double &d, double &dv, double &da) { lat_at(L, low_vel, tp, i, u_lowvel, d, dv, da); };
    double d_ext, dv_u, da_u;
    {
        const LonRow rl = row_at(traj_len - 1);
        lat_eval(traj_len - 1, rl.u1, d_ext, dv_u, da_u);
    }

    // ---- this lane's chunk of the horizon: fx_eval_kernel.h ----
    const int CH = G == 1 ? S : (S + G - 1) / G;
    const int i_begin = part * CH;
    const int i_end = min(S, i_begin + CH);
    const bool neigh = G == 32 && CH == 1;   // one step per lane: the left lane hands step i - 1 over (walk_step)
    const int i_first = (G > 1 && part > 0 && !neigh) ? i_begin - 1 : i_begin;

    StepConst K;
    fill_step_const<OBST>(K, P);
    K.low_vel = low_vel; K.dbg = dbg; K.do_collision = do_collision; K.store_wt = (P.mode & FX_MODE_INT_STORE_WT) != 0;
    K.atan_k = nullptr;
    const BoundView Bv{as_global(P.bound_piece), as_global(P.bound_bin), as_global(P.bound_item)};
    const FX_GLOBAL double *__restrict__ obs_rec = as_global(P.obs_rec);
    const FX_GLOBAL unsigned long long *__restrict__ obs_pmask = as_global(P.obs_pmask);
    const FX_GLOBAL unsigned long long *__restrict__ obs_hmask = as_global(P.obs_hmask);

    StepCarry Cy;
    Cy.reset(P.x0_orientation);
    auto moving_at = [&](int i) {   // a step's LON_MOVING bit: make_lon_row's own expression of the longitudinal velocity
        const double *te = tp + (i < traj_len ? i : traj_len - 1) * FX_TP;
        double sv = cl1 + 2. * cl2 * te[0] + 3. * cl3 * te[1] + 4. * cl4 * te[2] + 5. * cl5 * te[3];
        if (fabs(sv) < FX_EPS) sv = 0.0;
        return sv > 0.001;
    };
    unsigned long long moving_lanes = 0ULL;
    if (neigh) moving_lanes = __ballot(!low_vel && i_begin < S && moving_at(i_begin));
    if (G > 1 && !low_vel && i_first > 0 && i_first < S) {
        // the carry-in step keeps the previous heading when it stands still: scan back to the last moving step
        if (!moving_at(i_first)) {
            int j = i_first - 1;
            if (neigh) {   // the lanes are the candidate's steps: the last moving one in front of this from the ballot
                const unsigned int grp = (unsigned int)(moving_lanes >> ((tid & 63) & 32));
                const unsigned int below = grp & ((1u << part) - 1u);
                j = below ? 31 - __clz((int)below) : -1;
            } else {
                while (j >= 0 && !moving_at(j)) j--;
            }
            if (j >= 0) {
                const LonRow rj = row_at(j);
                double d_j, dv_j = 0.0, da_j;
                if (j < traj_len) lat_eval(j, rj.u1, d_j, dv_j, da_j);
                Cy.th_prev = heading_of_moving_step(rj, dv_j);
            }
        }
    }
    StepAcc A;
    A.reset();
    StepOut O;
    Simpson sim_acc, sim_jerk, sim_orient, sim_path;
    double a_prev = 0.0, thcl_prev = 0.0, dto = 0.0;
    if (EXTRA) { sim_acc.init(); sim_jerk.init(); sim_orient.init(); sim_path.init(); }
    const int n_dto = EXTRA ? P.n_dto : 0;
    const FX_GLOBAL double *__restrict__ dto_pos = as_global(P.dto_pos);
    bool lane_on = false;
    if (EXTRA)
        for (int q = 0; q < P.n_cost; q++) lane_on |= P.cost_id[q] == FX_COST_LANE_CENTER_OFFSET;
    double lane_off = 0.0;
    FX_GLOBAL double *__restrict__ planes = as_global(P.planes);
    const int64_t ps = (int64_t)S * ld;

#pragma unroll 1
    for (int i = i_first; i < i_end; i++) {
        const bool emit = i >= i_begin;  // false only for the carry-in step of parts > 0
        const LonRow r = row_at(i);
        walk_step<OBST, G == 1>(K, r, L, tp, i, traj_len, d_ext, emit, bundle && active && emit, planes + (int64_t)i * ld + g, 0u, ps, Cy, A, O,
                                obs_rec, obs_pmask, obs_hmask, Bv, nullptr, -1, neigh, part > 0);
        if (EXTRA) {   // the windowed terms: fx_eval_kernel.h, partial_cost_functions.py
            sim_acc.push(O.a * O.a, S);
            sim_path.push(O.v, S);
            if (i > 0) {
                const double j = (O.a - a_prev) / dt;
                const double w = (O.th_cl - thcl_prev) / dt;
                sim_jerk.push(j * j, S - 1);
                sim_orient.push(w * w, S - 1);
            }
            a_prev = O.a;
            thcl_prev = O.th_cl;
            for (int o = 0; o < n_dto; o++) {
                const double ex = O.x - dto_pos[2 * o], ey = O.y - dto_pos[2 * o + 1];
                const double dist = sqrt(ex * ex + ey * ey);
                dto += 1.0 / (dist * dist);
            }
            if (lane_on) lane_off += lane_center_distance(P, O.x, O.y);
        }
    }

    WalkResult W;
    W.neg = A.neg; W.acc_viol = A.acc_viol; W.collided = A.collided;
    W.step_reasons = A.step_reasons; W.first_key = A.first_key; W.fail_step = A.fail_step; W.bound_step = A.bound_step;
    W.sum_abs_d = A.sum_abs_d; W.sum_voff = A.sum_voff; W.pred = A.pred; W.dto = dto; W.lane_off = lane_off; W.d_end = A.d_end; W.v_end = A.v_end;
    W.set_poly(cl3, cl4, cl5, L);
    if (EXTRA) { W.sim_acc = sim_acc; W.sim_jerk = sim_jerk; W.sim_orient = sim_orient; W.sim_path = sim_path; }
    const FuseArgs no_fuse{nullptr, 0ULL, nullptr, 0};   // no fused selection, no tail: the outputs and the clone's own scratch only
    finish_candidate<G, true, OBST, EXTRA>(P, Pg, W, g, active, part, i_begin, i_end, bundle, do_collision, dbg, D, red_cost, red_idx, red_cnt,
                                           no_fuse);
}
