/*
 * fxplan.h -- C-ABI of libfxplan.so, the MI355X (gfx950) Frenet sampling-and-evaluation engine.
 *
 * The reference (TUM-AVS/Frenetix-Motion-Planner @ 2024_10_08) has no C-ABI: its hot path is
 * reached through the pybind11 module `frenetix` (C++ wheel, not in tree) that
 * frenetix_motion_planner/reactive_planner_cpp.py drives, or through the pure-Python
 * frenetix_motion_planner/reactive_planner.py.  This header is the boundary a maintainer binds
 * instead (ctypes stub: INTEGRATION.md).  Every entry point cites the reference interface it
 * replaces.  Plain pointers and sizes only; all floating point is IEEE binary64.
 *
 * Semantics follow the reference *Python* path (reactive_planner.py:132-577,
 * trajectories.py:524-561, cost_function.py:78-91, planner.py:329-392); the `frenetix` handler is
 * only the calling convention.  See DESIGN.md for the normative definitions of the two pieces
 * of third-party arithmetic that are not in the reference tree (curvilinear->Cartesian projection
 * and the OBB-sum collision test).
 */
#ifndef FXPLAN_H
#define FXPLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX_ABI_VERSION 15

/* ---- status codes (planner.py / reactive_planner_cpp.py raise Python exceptions; the shim maps
 *      <0 -> ValueError, >0 -> RuntimeError, see SURVEY 8b "Error conventions") ---- */
#define FX_OK 0
#define FX_ERR_INVALID_ARGUMENT (-1)
#define FX_ERR_NOT_READY (-2)     /* reference / vehicle / sampling not set before a plan step */
#define FX_ERR_CAPACITY (-3)      /* problem larger than the context was created for */
#define FX_ERR_HIP 1              /* a HIP runtime call failed; text in fx_last_error() */
#define FX_ERR_NO_DEVICE 2
#define FX_ERR_TIMEOUT 3          /* no answer from the device within the context's time bound (fx_set_timeout_ms): a peer that never
                                   * joined a collective or a faulted kernel.  The context refuses further steps; destroy it (and, in a
                                   * multi-rank job, end the process: a fresh child may be started, a process that touched the GPU is
                                   * never re-exec'ed).  The reference bounds its inter-process hand-offs the same way, TIMEOUT = 20 s:
                                   * cr_scenario_handler/simulation/simulation.py:637,655, agent_batch.py:98 */

/* ---- trajectory planes of the structure-of-arrays TrajectoryBundle.
 *      trajectories.py:56-197 (CartesianSample) and :200-334 (CurviLinearSample).
 *      Device layout: plane[p][step][ld] (ld = candidate count rounded up to 64), f64. ---- */
enum {
    FX_PL_X = 0, FX_PL_Y, FX_PL_THETA, FX_PL_V, FX_PL_A, FX_PL_KAPPA, FX_PL_KAPPA_DOT,
    FX_PL_S, FX_PL_D, FX_PL_THETA_CL, FX_PL_S_DOT, FX_PL_S_DDOT, FX_PL_D_DOT, FX_PL_D_DDOT,
    FX_NUM_PLANES
};

/* ---- partial cost functions (partial_cost_functions.py).  Ids are in alphabetical order of the
 *      reference names because cost_function.py:55-60 sorts the active names; callers list the
 *      active ids ascending. ---- */
enum {
    FX_COST_ACCELERATION = 0,            /* :24-33  */
    FX_COST_DISTANCE_TO_OBSTACLES,       /* :172-186 */
    FX_COST_DISTANCE_TO_REFERENCE_PATH,  /* :154-169 */
    FX_COST_JERK,                        /* :36-46  */
    FX_COST_LANE_CENTER_OFFSET,          /* :91-117 (needs the lanelets: FxProblem.n_lane ...; DESIGN.md 4.4, parity unpinned) */
    FX_COST_LATERAL_JERK,                /* :49-55  */
    FX_COST_LONGITUDINAL_JERK,           /* :58-64  */
    FX_COST_ORIENTATION_OFFSET,          /* :141-151 */
    FX_COST_PATH_LENGTH,                 /* :189-196 */
    FX_COST_PREDICTION,                  /* :341-356 + collision_probability.py:264-299 */
    FX_COST_VELOCITY_OFFSET,             /* :120-130 */
    FX_NUM_COSTS
};

/* ---- per-candidate flag word ---- */
#define FX_FLAG_VALID      (1u << 0)  /* reactive_planner.py:293,350-351,544 */
#define FX_FLAG_FEASIBLE   (1u << 1)  /* :292 and the five constraints :480-533 */
#define FX_FLAG_COLLISION  (1u << 2)  /* planner.py:348-357 (dynamic-obstacle prediction check) */
#define FX_FLAG_RETURNED   (1u << 3)  /* member of check_feasibility's return list (:353,379,385,567) */
#define FX_FLAG_COSTED     (1u << 4)  /* cost evaluated (:244-253: all returned in debug, feasible otherwise) */
#define FX_FLAG_SELECTABLE (1u << 5)  /* walked by trajectory_collision_check (:248,251,258) */
#define FX_FLAG_BOUNDARY   (1u << 6)  /* planner.py:362-381: the ego footprint leaves the road (boundary_harm != 0) */
#define FX_REASON_SHIFT 8             /* bits 8..18: reasons 0..10 flagged as in :352,378,384,418,485-531,545 */
#define FX_REASON_MASK  (0x7FFu << FX_REASON_SHIFT)
#define FX_NUM_REASONS 11

/* evaluation mode bits (configurations/frenetix_motion_planner/debug.yaml) */
#define FX_MODE_DRAW_TRAJ_SET   (1u << 0)  /* debug.draw_traj_set : evaluate everything, no pre-filter */
#define FX_MODE_KINEMATIC_DEBUG (1u << 1)  /* debug.kinematic_debug: keep checking after first violation */
#define FX_MODE_WRITE_BUNDLE    (1u << 2)  /* materialise the 14-plane SoA TrajectoryBundle in HBM */
#define FX_MODE_WRITE_COSTMAP   (1u << 3)  /* keep the per-name raw costs (TrajectorySample.costMap) */
#define FX_MODE_COLLISION       (1u << 4)  /* run the OBB collision stage (planner.use_prediction) */
#define FX_MODE_ROAD_BOUNDARY   (1u << 5)  /* test the ego footprint against the road boundary (planner.py:362-381) */
/* (s, d) -> (x, y) offsets d along the UN-normalised interpolated vertex normal (d is a pseudo-distance) instead of along its
 * unit vector -- the two readings of CCosy's construction differ by up to 7 mm on the ZAM_Tjunction route (DESIGN.md 4.1;
 * tests/golden/pin_third_party.py decides which one the reference's CCosy is, once commonroad_dc is importable) */
#define FX_MODE_PROJ_PSEUDO_NORMAL (1u << 6)

/* longitudinal sampling mode.
 * FX_LON_VELOCITY_KEEPING: v_samp = sampled end velocities, quartic to (v, 0) -- _create_trajectory_bundle,
 *   reactive_planner.py:132-182.
 * FX_LON_STOP_POINT: v_samp = sampled end POSITIONS s, quintic to (s, 0, 0) -- stop-point sampling,
 *   _create_end_point_trajectory_bundle, reactive_planner.py:628-671 (cpp: generate_stopping_trajectories,
 *   reactive_planner_cpp.py:258-290).  Ranges only (the C x 13 matrix has no end-position column). */
#define FX_MAX_OBSTACLES 256   /* predicted obstacles per agent (FxProblem.K) */
#define FX_LON_VELOCITY_KEEPING 0
#define FX_LON_STOP_POINT 1

/* vehicle parameters: configuration.py:58-83 (VehicleConfiguration); kappa_max is
 * tan(delta_max)/wheelbase as computed at reactive_planner.py:492 (host computes it once). */
typedef struct FxVehicle {
    double a_max, v_switch, delta_max, wheelbase, length, width, wb_rear_axle, kappa_max;
} FxVehicle;

/* Everything a plan step needs that is shared by all candidates of one agent.
 * reactive_planner.py:67-130 (plan), planner.py:172-217 (update_externals). */
typedef struct FxProblem {
    /* horizon: planner.py:63-65 */
    int32_t N;              /* steps; every trajectory has S = N+1 samples */
    double dt;
    uint32_t mode;          /* FX_MODE_* */
    int32_t low_vel_mode;   /* planner.py:222-230 */
    int32_t lon_mode;       /* FX_LON_*: what the longitudinal samples (v_samp) are */
    double x0_lon[3];       /* x_cl[0] = [s, s_dot, s_ddot]   planner.py:567-635 */
    double x0_lat[3];       /* x_cl[1] = [d, d_dot, d_ddot] */
    double x0_orientation;  /* x_0.orientation, used at reactive_planner.py:447 */
    double v_des;           /* desired_velocity (cost_function.py:70) */
    FxVehicle veh;

    /* time grid: t[i]=round(arange(0,..,dt),5) and its powers rounded to 10 dp
     * (reactive_planner.py:296-300).  tpow[k*S + i] = t_i^(k+1), k = 0..4, i = 0..S-1.
     * Host-computed with the reference's own expressions so the device never calls pow(). */
    const double *tpow;

    /* sampling: ordered ranges in *iteration order* (sampling_matrix.py:141-195; CPython set
     * order, reactive_planner.py:149-158).  Candidate g = (it*nV + iv)*nD + id.
     * v_samp holds end velocities or, with FX_LON_STOP_POINT, end positions (:641-643). */
    int32_t nT, nV, nD;
    const double *t_samp, *v_samp, *d_samp;
    /* ...or an explicit C x 13 matrix (sampling_matrix.py:85-121, reactive_planner_cpp.py:228-253)
     * when sampling_matrix != NULL; then nT/nV/nD are ignored and C = n_rows. */
    const double *sampling_matrix;
    int64_t n_rows;
    /* candidate shard [shard_begin, shard_begin + shard_count) of the global grid evaluated by this
     * context (multi-GPU candidate sharding); shard_count == 0 means the whole grid.
     * Per-candidate outputs are indexed locally (0..shard_count), best_index / top-k stay global so
     * that the (cost, index) tie-break is the same on every rank. */
    int64_t shard_begin, shard_count;

    /* reference path: utils_coordinate_system.py:189-207 (ref_pos/ref_theta/ref_curv/ref_curv_d),
     * plus vertices and vertex normals for the projection (DESIGN.md "projection"). */
    int32_t M;
    const double *ref_x, *ref_y, *ref_nx, *ref_ny, *ref_pos, *ref_theta, *ref_curv, *ref_curv_d;

    /* cost function: cost_function.py:40-64.  ids ascending (== name-sorted). */
    int32_t n_cost;
    const int32_t *cost_id;
    const double *cost_w;
    double simpson_corr[3]; /* alpha, beta, eta of scipy.integrate.simpson's even-N correction for h=[dt,dt] */

    /* predictions (prediction_helpers.py:209-261 dict -> packed): K obstacles, P steps each.
     * obs_pos[K][P][2], obs_cov_inv[K][P][4] (np.linalg.inv(cov_list), row-major 2x2),
     * obs_npred[K] = len(pos_list): the REAL length of the prediction -- it decides which ego steps see the obstacle
 * (collision_probability.py:287) and may exceed the stride P, which only bounds what is stored and read (a predictor with a longer
 * horizon than the planner's does not enlarge the tables; fx_pack_predictions).  collision_probability.py:264-299.
     * K <= FX_MAX_OBSTACLES; up to 64 obstacles the grid kernel applies, beyond that the step runs on the generic kernel
     * (the per-step obstacle masks take one 64-bit word per 64 obstacles). */
    int32_t K, P;
    const double *obs_pos, *obs_cov_inv;
    const int32_t *obs_npred;
    /* collision stage: OBB hulls of consecutive predicted boxes, obs_hull[K][P-1][6] =
     * (cx, cy, ex, ey, h1, h2) with unit axis e and half extents h; obs_nhull[K] = number of hulls
     * (0 when the obstacle is skipped, collision_check.py:165-168).  Built by fx_build_obstacle_hulls. */
    const double *obs_hull;
    const int32_t *obs_nhull;
    /* distance_to_obstacles cost: obstacle positions at the current step, dto_pos[n_dto][2]
     * (partial_cost_functions.py:179-184). */
    int32_t n_dto;
    const double *dto_pos;
    /* road boundary (planner.py:362-381; built once per scenario, :550-565): n_bound straight pieces
     * bound_piece[n_bound][4] = (mid x, mid y, half dx, half dy), and per reference knot k the pieces that can
     * touch an ego footprint whose foot point lies on segment k: bound_item[bound_bin[k] .. bound_bin[k+1])
     * (CSR, M+1 offsets).  Built by fx_build_boundary_bins.  DESIGN.md 4.3 is the normative test. */
    int32_t n_bound;
    const double *bound_piece;
    const int32_t *bound_bin;
    const int32_t *bound_item;
    double bound_d_reach;   /* lateral reach the bins were built for; |d| beyond it counts as off the road */
    /* lane_center_offset cost (partial_cost_functions.py:91-117): the lanelets in network order.  Per trajectory point the
     * FIRST lanelet whose outline contains it (lane_poly[lane_poly_off[l] .. lane_poly_off[l+1]) = left vertices, then the
     * right ones reversed; ray casting; lane_bbox[l] = (x min, x max, y min, y max) settles most lanelets) and the distance
     * to that lanelet's centre polyline lane_ctr[lane_ctr_off[l] .. lane_ctr_off[l+1]) -- the closest point of its segments;
     * 5 when no lanelet contains the point; the cost is the mean over the trajectory's points.  The reference asks
     * commonroad-io (find_lanelet_by_position) and shapely (project / interpolate), neither of which is in the reference
     * tree: which lanelet is "first" where lanelets overlap, and points exactly on an outline, are this header's definition. */
    int32_t n_lane;
    const double *lane_bbox;       /* [n_lane][4] */
    const int32_t *lane_poly_off;  /* [n_lane + 1] */
    const double *lane_poly;       /* [lane_poly_off[n_lane]][2] */
    const int32_t *lane_ctr_off;   /* [n_lane + 1] */
    const double *lane_ctr;        /* [lane_ctr_off[n_lane]][2] */
} FxProblem;

/* Result of one plan step (what _get_optimal_trajectory returns plus the counters it sets,
 * reactive_planner.py:184-272; planner.py:329-392). */
typedef struct FxResult {
    int64_t n_candidates;
    int64_t best_index;        /* uniqueId of the selected trajectory, -1 if none */
    double best_cost;
    int64_t n_returned;        /* len(trajectories_all) */
    int64_t n_feasible;        /* len(feasible_trajectories) (valid and feasible) */
    int64_t n_infeasible;      /* _infeasible_count_kinematics[0] */
    int64_t n_collisions;      /* _collision_counter: colliding candidates walked before the winner */
    int64_t reason_hist[FX_NUM_REASONS]; /* infeasible_invalid_count_kinematics (queue_2 payload) */
    double feasible_percentage;/* infeasible_kinematics_percentage (is the feasible %, :235) */
    double kernel_ms;          /* HIP-event time of the device work of this step; -1 when the step was not timed or
                                * its events were still pending when fx_finish returned (fx_last_kernel_ms waits) */
} FxResult;

typedef struct FxContext FxContext;

/* ---- library ---- */
int32_t fx_abi_version(void);
const char *fx_last_error(void);          /* thread-local text of the last failure */
int32_t fx_device_count(int32_t *count);  /* no context needed */

/* ---- context: owns device buffers sized for up to max_candidates x (max_steps+1); one per
 *      planner instance (frenetix.TrajectoryHandler(dt=) at reactive_planner_cpp.py:49).
 *      stream: a hipStream_t as void* (0 -> the context creates its own).
 *      A create that fails stores NULL in *out and has given back everything it had built: there is nothing to destroy. ---- */
int32_t fx_create(FxContext **out, int32_t device, int64_t max_candidates, int32_t max_steps,
                  int32_t max_ref_knots, int32_t max_obstacles, int32_t max_pred_steps);
int32_t fx_destroy(FxContext *ctx);
int32_t fx_set_stream(FxContext *ctx, void *hip_stream);
/* tuning override (0 = automatic): lanes that share one candidate's horizon (1, 2, 4, 8, 16, 32), the occupancy
 * target in waves per SIMD (2..4) of the evaluation kernel, and the kernel variant (1 = generic per-candidate
 * kernel, 2 = grid kernel with the per-(t,v) longitudinal table).  Results do not depend on any of them. */
int32_t fx_set_tuning(FxContext *ctx, int32_t lanes_per_candidate, int32_t waves_per_simd, int32_t kernel_variant);
/* device buffer [n_agents][2] = (cost f64, global index i64) that every evaluated step also leaves its winner in,
 * so a k = 1 survivor exchange needs no extra kernel (NULL to disable); e.g. a torch tensor's data_ptr() */
int32_t fx_set_winner_buffer(FxContext *ctx, void *d_winner);
/* publish n doubles of a small device buffer (the all-gathered survivors) to the host through pinned memory on the
 * context stream, and wait for / copy them out: avoids a D2H copy + stream synchronisation per step */
int32_t fx_publish(FxContext *ctx, const void *d_src, int32_t n);
int32_t fx_wait_published(FxContext *ctx, double *out);
/* how the parts of a split horizon map to lanes: 0 auto, 1 adjacent lanes (shuffle combine), 2 lane-groups of the
 * workgroup ("wave split", LDS combine; keeps every plane store a contiguous row segment per wave) */
int32_t fx_set_part_mapping(FxContext *ctx, int32_t mapping);
/* workgroup size of the grid kernel: 0 (auto), 64, 128 or 256 lanes */
int32_t fx_set_block_size(FxContext *ctx, int32_t block_size);
/* how the bundle's plane stores leave the CU: 0 auto (by bundle size), 1 plain write-back stores, 2 write-through
 * (agent-scope) stores -- nothing dirty is left in the L2s for the end-of-kernel write-back, which pays off while the
 * whole bundle is small (measured on MI355X: 42 vs 45 us at 175 MB, 780 vs 650 us at 3.5 GB).  Results are unaffected. */
int32_t fx_set_store_mode(FxContext *ctx, int32_t store_mode);

/* where the obstacle stage (prediction cost collision_probability.py:264-299 + OBB-sum collision walk planner.py:329-392) runs:
 * 0 auto, 1 fused into the horizon walk, 2 as its own (candidate x step)-parallel kernel behind the walk -- it reads x / y /
 * theta back from the materialised planes, so it needs FX_MODE_WRITE_BUNDLE, at most 64 obstacles, no road-boundary stage and
 * no windowed cost term (FX_ERR_INVALID_ARGUMENT at the next upload otherwise).  steps_per_item (0 auto, 2, 3, 5): horizon steps
 * one wave of that kernel visits.  Decisions (flags, counters, winner) do not depend on either; the prediction cost is summed
 * in a different order (agreement 1e-13 relative). */
int32_t fx_set_obstacle_stage(FxContext *ctx, int32_t stage, int32_t steps_per_item);

/* ---- staging: copy the shared inputs of a plan step to the device (borrowed for the call).
 *      Replaces handler.generate_trajectories(matrix, low_vel_mode) + the functor registration
 *      at reactive_planner_cpp.py:96-178,256. ---- */
int32_t fx_upload(FxContext *ctx, const FxProblem *prob);

/* ---- evaluation: fused sample -> solve -> evaluate -> Frenet->Cartesian -> feasibility -> cost
 *      -> collision launch plus the (cost, index) selection.  Replaces
 *      handler.evaluate_all_current_functions(True) (:347-349) and, in the Python path,
 *      check_feasibility + TrajectoryBundle.sort + trajectory_collision_check.
 *      fx_evaluate only enqueues on the context stream; fx_finish synchronises and fills *res. ---- */
int32_t fx_evaluate(FxContext *ctx);
int32_t fx_finish(FxContext *ctx, FxResult *res);
/* convenience: upload + evaluate + finish */
int32_t fx_plan_step(FxContext *ctx, const FxProblem *prob, FxResult *res);
/* evaluate + finish for inputs that are already resident (the handler re-evaluating its current trajectory set,
 * reactive_planner_cpp.py:345-349): one call across the boundary per plan step; res[n_agents] */
int32_t fx_step(FxContext *ctx, FxResult *res);

/* ---- per-step update of a planner that keeps its reference path, grid shape and cost function: the new ego state,
 *      desired velocity, sampling values and predictions of planner.py:172-217 (update_externals) / reactive_planner_cpp.py:
 *      56-86 (set_predictions) rewritten in place in the context's pinned staging block; the range that
 *      changed is staged in front of the next evaluation (a copy kernel reading the mapped block; the DMA engine above 1 MiB).  NULL pointers, NaN doubles and a negative low_vel_mode keep the uploaded
 *      value; array lengths (nT, nV, nD, K, P) are those of the upload.  fx_update_step = fx_update_state(agent 0) + fx_step. */
typedef struct FxStateUpdate {
    const double *x0_lon, *x0_lat;             /* [3] each */
    double x0_orientation, v_des;
    int32_t low_vel_mode;
    const double *t_samp, *v_samp, *d_samp;
    const double *obs_pos, *obs_cov_inv;       /* [K][P][2], [K][P][4] */
    const int32_t *obs_npred;                  /* [K] */
    const double *obs_hull;                    /* [K][P-1][6] */
    const int32_t *obs_nhull;                  /* [K] */
    /* the array shapes as the CALLER holds them (0 = not stated, nothing is checked): the library copies nT / nV / nD doubles and
     * K x P obstacle rows out of the borrowed pointers with the counts of the UPLOAD -- a caller whose arrays were built for another
     * grid or another (K, P) would be read past their end.  A stated count that differs from the upload's is refused with
     * FX_ERR_INVALID_ARGUMENT before anything is rewritten (upload again). */
    int32_t nT, nV, nD, K, P;
} FxStateUpdate;
int32_t fx_update_state(FxContext *ctx, int32_t agent, const FxStateUpdate *upd);
int32_t fx_update_step(FxContext *ctx, const FxStateUpdate *upd, FxResult *res);

/* ---- multi-GPU survivor exchange inside the library (one process per GPU; the reference fans candidate chunks / agent batches
 *      out to processes and pickles results back through Queues, reactive_planner.py:197-224, simulation.py:449-470) ----
 *      The context gets an RCCL communicator of its own: rank 0 draws the 128-byte id (fx_comm_unique_id), the host program
 *      broadcasts it by whatever means it has, every rank calls fx_comm_init.  fx_step_exchange = fx_evaluate + ONE all-gather of
 *      every rank's winner (cost f64, global index i64) per agent on the context's stream + publication to pinned host memory +
 *      fx_finish_batch: cost / index [world][agent rows], index -1 where a rank found nothing.  RCCL is bound at run time
 *      (librccl.so.1); without it these return FX_ERR_NOT_READY and everything else works. */
int32_t fx_comm_unique_id(uint8_t *id128);
/* local preconditions of fx_comm_init (RCCL present, capacity) WITHOUT entering anything collective: every rank calls it and the
 * ranks agree (all-reduce MIN over the host program's own group) before any of them calls fx_comm_init -- a rank that would fail
 * there never reaches ncclCommInitRank and its peers would wait for it forever */
int32_t fx_comm_check(const FxContext *ctx, int32_t world);
int32_t fx_comm_init(FxContext *ctx, const uint8_t *id128, int32_t rank, int32_t world);
int32_t fx_comm_destroy(FxContext *ctx);
/* the agent rows EVERY rank contributes to an exchange (default: the context's max_agents).  The element count of the all-gather
 * is a property of the communicator, agreed between the ranks and fixed here -- not of a rank's current upload: a rank that
 * uploaded fewer agents sends "no survivor" (inf, -1) in the remaining rows, a rank that uploaded more gets FX_ERR_CAPACITY
 * from the exchange (after having entered it) */
int32_t fx_comm_set_agents(FxContext *ctx, int32_t n_agents);
/* where the exchanges' all-gather lands: 0 (default) a device buffer + the publication kernel, 1 straight in the pinned, mapped
 * block with a stream-ordered write of the sequence word (no launch behind the collective).  Use mode 1 only after it has
 * agreed with an independent exchange on every rank (distributed.ShardedEvaluator does that). */
int32_t fx_set_exchange_mode(FxContext *ctx, int32_t mode);
/* out[0] rank, [1] world, [2] the ranks RCCL itself reports for the communicator (ncclCommCount, -1 if unavailable), [3] agent
 * rows per rank */
int32_t fx_comm_info(const FxContext *ctx, int32_t *out4);
/* A = the communicator's agent rows (fx_comm_set_agents).  A rank whose own evaluation fails, or whose upload does not fit A
 * rows, still enters the all-gather (with cost inf / index -1 in its rows) and returns its error afterwards: nothing that can
 * fail locally returns ahead of the collective, the peers are never left waiting */
int32_t fx_step_exchange(FxContext *ctx, FxResult *res, double *cost /*[world][A]*/, int64_t *index /*[world][A]*/);
/* the same for the k <= 64 best survivors per agent (agent sharding with a top-k gather, BASELINE config 5): evaluation,
 * selection, top-k, ONE all-gather of 16 k bytes per rank and agent row, publication -- no host code between the launches; k is
 * the same on every rank */
int32_t fx_step_exchange_topk(FxContext *ctx, int32_t k, FxResult *res, double *cost /*[world][A][k]*/,
                              int64_t *index /*[world][A][k]*/);
/* every host wait on device work (fx_finish, fx_wait_published, the exchanges, fx_read_package) is bounded in TIME: default
 * 20 000 ms, the reference's TIMEOUT (simulation.py:637); FX_ERR_TIMEOUT when it runs out.  fx_wait_word is the wait itself
 * (pure host code): returns FX_OK once *word == expected, FX_ERR_TIMEOUT after timeout_ms. */
int32_t fx_set_timeout_ms(FxContext *ctx, int32_t timeout_ms);
int32_t fx_wait_word(const volatile unsigned long long *word, unsigned long long expected, int32_t timeout_ms);

/* ---- the chosen trajectory, packaged (planner.py:394-447 _compute_trajectory_pair; reactive_planner_cpp.py:355-357 reads the
 *      optimal trajectory's arrays; frenet_interface.py:243-277 consumes the pair) ----
 *      With fx_set_package(ctx, 1) every evaluation that writes the bundle is followed by a gather of the winner's data into
 *      pinned host memory on the same stream, and fx_finish returns once it has arrived: no strided read-back, no second
 *      synchronisation.  fx_read_package hands it out: `pkg` = index (global), cost, flag word, horizon, coefficients, raw
 *      partial costs; `block` (may be NULL) = [FX_PKG_ROWS][S] doubles: the FX_NUM_PLANES planes in PLANE order, then
 *      yaw_rate (yaw_rate0, then backward differences of theta over dt), steering_angle atan2(wheelbase * kappa, 1) and the
 *      heading shifted into [x0_orientation - pi, x0_orientation + pi].  found = 0: no selectable collision-free candidate.
 *      fx_plan_and_package = fx_update_state(agent 0, upd; upd may be NULL) + fx_evaluate + fx_finish + fx_read_package in ONE
 *      call: a planner's closed-loop plan step. */
#define FX_PKG_ROWS (FX_NUM_PLANES + 3)
typedef struct FxPackage {
    int32_t found, S, traj_len;
    uint32_t flags;
    int64_t index;
    double cost;
    double coeff_lon[6], coeff_lat[6];
    int32_t n_cost, reserved;
    double raw_costs[FX_NUM_COSTS];
    double tau_lat;   /* delta_tau of the lateral polynomial: t, or in LOW_VEL_MODE s_lon_goal (reactive_planner.py:161-171, :650-659);
                       * the longitudinal polynomial's delta_tau is always t = sampling_parameters[1] - [0] */
} FxPackage;
int32_t fx_set_package(FxContext *ctx, int32_t enabled);
int32_t fx_read_package(FxContext *ctx, int32_t agent, double yaw_rate0, FxPackage *pkg, double *block /*[FX_PKG_ROWS][S] or NULL*/);
int32_t fx_plan_and_package(FxContext *ctx, const FxStateUpdate *upd, double yaw_rate0, FxResult *res, FxPackage *pkg, double *block);
/* the plan steps of a batch of agents in ONE call (agent_batch.py:140-189 runs one planner after the other): fx_update_state for
 * every agent whose upd[a] is not NULL (upd itself may be NULL), one evaluation with the winner package on, the results, every
 * agent's package.  n_agents = the uploaded batch's; yaw_rate0 [n_agents] (NULL: zeros); blocks [n_agents] pointers to
 * [FX_PKG_ROWS][S_a] doubles each (NULL, or NULL entries: no block).  A refused update leaves the context as the earlier
 * agents' updates left it and nothing is evaluated. */
int32_t fx_plan_batch_packaged(FxContext *ctx, int32_t n_agents, const FxStateUpdate *const *upd, const double *yaw_rate0, FxResult *res,
                               FxPackage *pkg, double *const *blocks);
/* the same in two halves, so that a host with several contexts keeps one evaluating while it prepares the next one's inputs and
 * consumes the previous one's results: _begin = the state updates + the evaluation's launches (returns without waiting),
 * _end = the wait, the results and the packages of THAT evaluation. */
int32_t fx_plan_batch_begin(FxContext *ctx, int32_t n_agents, const FxStateUpdate *const *upd);
int32_t fx_plan_batch_end(FxContext *ctx, int32_t n_agents, const double *yaw_rate0, FxResult *res, FxPackage *pkg, double *const *blocks);

/* ---- host geometry of the callers either side of the path (plain C, no device) ----
 *      fx_cs_to_curvilinear: (s, d) of a Cartesian point along a reference polyline with per-vertex normals (the projection
 *      behind planner.py:574-578); ref_xy / normals [M][2], ref_pos [M]; FX_ERR_INVALID_ARGUMENT outside the projection domain.
 *      fx_build_obstacle_hulls_batch: fx_build_obstacle_hulls for K obstacles stored with stride P. */
int32_t fx_cs_to_curvilinear(int32_t M, const double *ref_xy, const double *normals, const double *ref_pos, double x, double y,
                             double *sd /*[2]*/);
/* the same with the projection variant spelled out: pseudo_normal != 0 inverts the FX_MODE_PROJ_PSEUDO_NORMAL map */
int32_t fx_cs_to_curvilinear_ex(int32_t M, const double *ref_xy, const double *normals, const double *ref_pos, double x, double y,
                                int32_t pseudo_normal, double *sd);
/* n 2x2 matrices (row-major, 4 doubles each) inverted with the arithmetic of np.linalg.inv, bit for bit (collision_probability.py:281) */
int32_t fx_invert_cov2(int32_t n, const double *m, double *out);
/* K predicted obstacles -> the obstacle arrays of FxProblem / FxStateUpdate in one call (covariance inverses, hulls, padding
 * to the stride P); pos[k] [n[k]][2], cov[k] [n[k]][4], yaw[k] [n[k]] or NULL (no hulls for that obstacle). */
int32_t fx_pack_predictions(int32_t K, int32_t P, int32_t n_samples, const int32_t *n, const double *const *pos, const double *const *cov,
                            const double *const *yaw, const double *length, const double *width, double *pos_out, double *cov_inv_out,
                            int32_t *npred, double *hull, int32_t *nhull);
int32_t fx_build_obstacle_hulls_batch(int32_t K, int32_t P, const int32_t *n_use, const double *pos, const double *yaw,
                                      const double *length, const double *width, double *hull, int32_t *n_hull);

/* ---- read-back (TrajectorySample views are materialised lazily from the SoA bundle;
 *      reactive_planner_cpp.py:353 get_sorted_trajectories, trajectories.py:337-477) ---- */
int32_t fx_read_costs(FxContext *ctx, double *cost /*[C]*/, uint32_t *flags /*[C]*/);
int32_t fx_read_costmap(FxContext *ctx, double *raw /*[n_cost][C]*/);
int32_t fx_read_coeffs(FxContext *ctx, int64_t index, double *lon6, double *lat6, int32_t *traj_len);
int32_t fx_read_sample(FxContext *ctx, int64_t index, double *planes /*[FX_NUM_PLANES][S]*/);
int32_t fx_read_plane(FxContext *ctx, int32_t plane, double *out /*[S][C]*/);
/* k best selectable, collision-free candidates in (cost, index) order; returns count in *n_out.
 * Used for the host-side road-boundary walk (planner.py:362-390) and the multi-GPU exchange. */
int32_t fx_read_topk(FxContext *ctx, int32_t k, double *cost, int64_t *index, int32_t *n_out);
/* same, but left in device memory (caller-provided device pointers, e.g. torch tensors) so the
 * survivors can go straight into an RCCL all-gather; enqueued on the context stream. */
int32_t fx_topk_to_device(FxContext *ctx, int32_t k, void *d_cost /*f64[k]*/, void *d_index /*i64[k]*/);

/* ---- host-side helpers (pure CPU, no context) ---- */
/* OBB hulls of consecutive predicted boxes (collision_check.py:170-186 create_tvobstacle +
 * trajectory_preprocess_obb_sum; normative definition in DESIGN.md). pos[P][2], yaw[P]. */
int32_t fx_build_obstacle_hulls(int32_t n_pred, const double *pos, const double *yaw,
                                double length, double width, double *hull /*[n_pred-1][6]*/,
                                int32_t *n_hull);

/* ---- multi-agent batching: several agents evaluated by ONE launch (grid.y = agent).  The reference steps
 *      agents sequentially inside AgentBatch processes (cr_scenario_handler/simulation/agent_batch.py:186-189,
 *      simulation.py:449-470); agents are independent given the frozen predictions, so the batch is a pure
 *      concatenation.  max_candidates_total bounds the sum over agents.  res[n_agents]. ---- */
int32_t fx_create_batch(FxContext **out, int32_t device, int32_t max_agents, int64_t max_candidates_total,
                        int32_t max_steps, int32_t max_ref_knots, int32_t max_obstacles, int32_t max_pred_steps);
int32_t fx_upload_batch(FxContext *ctx, int32_t n_agents, const FxProblem *probs);
int32_t fx_finish_batch(FxContext *ctx, FxResult *res);
int32_t fx_read_costs_agent(FxContext *ctx, int32_t agent, double *cost, uint32_t *flags);
int32_t fx_read_costmap_agent(FxContext *ctx, int32_t agent, double *raw);
int32_t fx_read_coeffs_agent(FxContext *ctx, int32_t agent, int64_t index, double *lon6, double *lat6, int32_t *traj_len);
/* PolynomialTrajectory.delta_tau of one candidate's LATERAL polynomial as the device used it (polynomial_trajectory.py:17-60):
 * the sampled t, or -- LOW_VEL_MODE -- the arc length s_lon_goal = s(t) - s(0) of its longitudinal polynomial, t when that is
 * not positive (reactive_planner.py:161-171; stop-point bundle :650-659) */
int32_t fx_read_lat_tau_agent(FxContext *ctx, int32_t agent, int64_t index, double *tau_lat);
int32_t fx_read_sample_agent(FxContext *ctx, int32_t agent, int64_t index, double *planes);
int32_t fx_read_plane_agent(FxContext *ctx, int32_t agent, int32_t plane, double *out);
/* Everything a trajectory object of ONE candidate exposes (frenetix TrajectorySample: cartesian / curvilinear arrays,
 * coefficients, costMap, cost, feasibility -- reactive_planner_cpp.py:355-357,456,470-482) in one call with one stream
 * synchronisation: planes [FX_NUM_PLANES][S], coeffs13 = lon[6] | lat[6] | tau_lat (fx_read_lat_tau_agent), traj_len, raw partial costs [n_cost], total
 * cost and flag word.  Any output pointer may be NULL.  What the planner reads back for the chosen trajectory. */
int32_t fx_read_candidate_agent(FxContext *ctx, int32_t agent, int64_t index, double *planes, double *coeffs13,
                                int32_t *traj_len, double *raw_costs, double *cost, uint32_t *flags);
/* fx_read_candidate_agent for n candidates of one agent in one call -- what the reference's adapter asks of every evaluated
 * trajectory each plan step (reactive_planner_cpp.py:353-358) and what a planner keeps across steps (:430, 437: optimal_trajectory,
 * all_traj) -- in the caller's order (unsorted lists and duplicates are legal).  A gather kernel behind the step packs one record
 * per listed candidate (planes | lon lat tau_lat | raw costs | cost | traj_len | flags | boundary_step) into a device buffer, one
 * asynchronous copy brings it to pinned memory, one stream synchronisation -- per chunk of FX_READ_CHUNK_BYTES (the indices travel
 * in the same chunk: 8 bytes per candidate on top of its record), so the number of synchronisations is
 * ceil(n / floor(FX_READ_CHUNK_BYTES / (record bytes + 8))): 1 for everything a planner-sized step holds (800 candidates x 3.7 KB).
 * The two chunk buffers (device and pinned) are allocated on the first call.  Any output pointer may be NULL.  Same contract as
 * fx_read_candidate_agent: FX_ERR_NOT_READY where a requested part was not produced by the step (boundary_step: FX_MODE_ROAD_BOUNDARY),
 * FX_ERR_INVALID_ARGUMENT for n < 0, ids == NULL with n > 0 or any index outside [0, C) -- checked before anything is launched or
 * written; n == 0 returns FX_OK without device work. */
#define FX_READ_CHUNK_BYTES (8u << 20)
int32_t fx_read_candidates_agent(FxContext *ctx, int32_t agent, int64_t n, const int64_t *ids,
                                 double *planes        /* [n][FX_NUM_PLANES][S] or NULL */,
                                 double *coeffs13      /* [n][13]: lon[6] | lat[6] | tau_lat, or NULL */,
                                 int32_t *traj_len     /* [n] or NULL */,
                                 double *raw_costs     /* [n][n_cost] or NULL */,
                                 double *cost          /* [n] or NULL */,
                                 uint32_t *flags       /* [n] or NULL */,
                                 int32_t *boundary_step/* [n] or NULL */);
int32_t fx_read_topk_batch(FxContext *ctx, int32_t k, double *cost /*[n_agents][k]*/, int64_t *index /*[n_agents][k]*/);

/* ---- listed candidates of a plan step, materialised beside it -- DESIGN.md section 14; ABI 13 ----
 *      A step without FX_MODE_WRITE_BUNDLE (the throughput mode) hands back cost, flag word and index per candidate.  What a planner
 *      needs afterwards is a few dozen trajectories: the winner, the top-k survivors of its host walk (planner.py:362-390), the
 *      samples it keeps.  fx_materialise_candidates_agent re-walks a list of candidates of the last evaluated step of `agent` with
 *      the step's own arithmetic (the list form of the generic evaluation kernel, one lane per candidate, obstacle stage and road
 *      boundary in the walk) and stores their bundle rows, coefficients, horizon lengths, raw costs, costs, flag words and boundary
 *      steps in a compact block of the agent's own, the "sparse set".  It writes nothing a plan step wrote or published.
 *      ids: local indices in [0, C), any order, duplicates legal; the library keeps the set ascending and de-duplicated.  The call
 *      enqueues on the context's stream and returns; the readers below synchronise.  The set is valid until the next call for that
 *      agent or the next evaluation, upload or state update of the context; n == 0 clears it without device work.  The block is
 *      allocated on the first call and only grows: a context that never calls this owns what it always did (fx_device_bytes).
 *      FX_ERR_INVALID_ARGUMENT for n < 0, ids == NULL with n > 0, an index outside [0, C); FX_ERR_NOT_READY before the first
 *      evaluated step and when the resident inputs were rewritten since it (fx_upload*, or fx_update_state without an evaluation:
 *      the re-walk would use another state); FX_ERR_CAPACITY for a reference whose knots do not fit the generic kernel's LDS --
 *      all checked before anything is launched or written, a refused call leaves the previous set as it was. */
int32_t fx_materialise_candidates_agent(FxContext *ctx, int32_t agent, int64_t n, const int64_t *ids);
/* fx_read_candidates_agent on the sparse set: the same outputs, the same chunking, rows in the caller's order (unsorted lists and
 * duplicates are legal).  Every part is there whatever the step's mode was, except boundary_step, which needs
 * FX_MODE_ROAD_BOUNDARY.  FX_ERR_NOT_READY when a listed candidate is not in the agent's set (or there is no valid set). */
int32_t fx_read_materialised_agent(FxContext *ctx, int32_t agent, int64_t n, const int64_t *ids,
                                   double *planes        /* [n][FX_NUM_PLANES][S] or NULL */,
                                   double *coeffs13      /* [n][13] or NULL */,
                                   int32_t *traj_len     /* [n] or NULL */,
                                   double *raw_costs     /* [n][n_cost] or NULL */,
                                   double *cost          /* [n] or NULL */,
                                   uint32_t *flags       /* [n] or NULL */,
                                   int32_t *boundary_step/* [n] or NULL */);
/* the package of fx_read_package for candidate `index` (local) of the sparse set: found = 1, pkg->index global, block as there */
int32_t fx_read_package_materialised(FxContext *ctx, int32_t agent, int64_t index, double yaw_rate0, FxPackage *pkg,
                                     double *block /*[FX_PKG_ROWS][S] or NULL*/);
/* device time of the context's last materialise call, from the start of its first list-kernel launch to the end of its last
 * (events attached to the kernels), ms; -1 before the first.  Waits for it. */
double fx_last_materialise_ms(FxContext *ctx);
/* ---- the list pass on split lanes and for a whole agent batch -- DESIGN.md section 22; additive, the ABI version stays ----
 *      fx_set_materialise_lanes: lanes per listed candidate of the list kernel.  0 or 1 (the default): one lane walks a
 *      candidate's whole horizon; 8 or 32: the horizon is cut into that many chunks walked by adjacent lanes, the decomposition
 *      of the plan step's generic kernel at that many lanes, so a row equals the row that kernel stores bit for bit.  Anything
 *      else: FX_ERR_INVALID_ARGUMENT, and the setting stays.  It applies to fx_materialise_candidates_agent and to the batch
 *      call; an agent with a windowed cost term (acceleration, jerk, path_length, orientation_offset, distance_to_obstacles,
 *      lane_center_offset) runs at one lane whatever is set.  fx_set_tuning does not touch it. */
int32_t fx_set_materialise_lanes(FxContext *ctx, int32_t lanes);
/*      fx_materialise_candidates_batch: fx_materialise_candidates_agent for n_agents agents in one call -- agents[j] (NULL:
 *      agent j) with the list ids[j] of n_ids[j] candidates -- with one wait for the stream, one upload (row table, clones and
 *      lists) and one launch per kernel variant (lanes, obstacle stage, windowed terms) present among the agents, four at most.
 *      Each agent receives the set the per-agent call would have made, in its own block; the readers and the risk passes do not
 *      tell the two apart.  n_ids[j] == 0 clears that agent's set.  Everything is checked before anything is written or
 *      launched, and a refused call leaves every previous set readable and takes no memory: the per-agent refusals of each
 *      agent, and FX_ERR_INVALID_ARGUMENT for n_agents < 0 or more agents than the last upload holds, an agent outside it or
 *      listed twice, NULL n_ids or ids with n_agents > 0.  n_agents == 0 returns FX_OK and touches nothing. */
int32_t fx_materialise_candidates_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /* NULL: 0 ... n_agents - 1 */,
                                        const int64_t *n_ids, const int64_t *const *ids);
/*      the last materialise call of the context: the widest lane split among its rows, its list-kernel launches and its rows
 *      (agents with a non-empty list); zeros before the first and behind a call that only cleared.  Any pointer may be NULL. */
int32_t fx_last_materialise_info(FxContext *ctx, int32_t *lanes, int32_t *launches, int32_t *rows);

/* ---- stable cost order of ALL candidates of a plan step, sorted beside it and read back by rank -- DESIGN.md section 15 ----
 *      TrajectoryBundle.sort (trajectories.py:524-561) on the device: a stable radix sort of one agent's candidates by cost, ties
 *      and NaNs in index order, NaNs last -- np.argsort(kind="stable") of the pool's costs.  The pool is
 *      (flags & require) == require && (flags & exclude) == 0: require = FX_FLAG_COSTED, exclude = 0 is the reference's sorted
 *      list; require = FX_FLAG_SELECTABLE, exclude = FX_FLAG_COLLISION | FX_FLAG_BOUNDARY the top-k's survivors without its bound of
 *      64 (the top-k skips NaN costs: here they are the last n_nan ranks); 0, 0 every candidate.  *n_pool receives the pool's size,
 *      *n_nan the pool members with a NaN cost.  The calls launch on the context's stream and wait for the counts.  They read the
 *      cost and flag planes and write a block of their own -- nothing a plan step, the top-k, a sparse set or the risk passes own --
 *      which is allocated on the first call and only grows: a context that never sorts owns what it always did (fx_device_bytes).
 *      An order is valid until the next sort of that agent or the next evaluation, upload or state update of the context.
 *      FX_ERR_NOT_READY before the first evaluated step, when the inputs were rewritten since it, and for the two readers without
 *      a valid order; FX_ERR_INVALID_ARGUMENT for NULL where a pointer is needed, an agent out of range, first < 0, n < 0 or
 *      first + n > n_pool -- all checked before anything is launched or written: a refused call leaves the previous order
 *      readable.  n == 0 is legal. */
int32_t fx_sort_candidates_agent(FxContext *ctx, int32_t agent, uint32_t require, uint32_t exclude, int64_t *n_pool, int64_t *n_nan);
/* every agent of the last step in ONE launch sequence (agents are grid.y), each within its own segment */
int32_t fx_sort_candidates_batch(FxContext *ctx, uint32_t require, uint32_t exclude, int64_t *n_pool /*[n_agents]*/,
                                 int64_t *n_nan /*[n_agents]*/);
/* ranks [first, first + n) of the agent's last sort: LOCAL indices in [0, C) -- the convention of fx_read_candidates_agent and
 * fx_materialise_candidates_agent, which a rank range feeds directly -- and, where asked for, cost[index] and flags[index] gathered
 * from the agent's planes: the bits as the step wrote them (costs are never rebuilt from sort keys). */
int32_t fx_read_ranked_agent(FxContext *ctx, int32_t agent, int64_t first, int64_t n, int64_t *index /*[n]*/,
                             double *cost /*[n] or NULL*/, uint32_t *flags /*[n] or NULL*/);
/* device pointer of the agent's order, int64 local indices by rank ([0, *n_pool) are the pool), for callers that stay on the GPU */
int32_t fx_sort_views(FxContext *ctx, int32_t agent, void **d_index, int64_t *n_pool);
/* device time of the context's last sort (events around its launches), ms; -1 before the first.  Waits for it. */
double fx_last_sort_ms(FxContext *ctx);

/* ---- a finished plan step re-scored under many cost-weight vectors at once, beside the step -- DESIGN.md section 23; additive
 *      within ABI 15 ----
 *      update_externals(cost_weights=...) (planner.py:204-205, reactive_planner_cpp.py:88-94) asked of a step that has already run:
 *      which candidate wins under these other weights?  w[n_vec][n_cost] are weight vectors over the step's own cost list (its
 *      non-zero terms in ascending id order).  total(c) under a vector is what the step would have stored as cost[c] had it run with
 *      it -- the same multiplications and additions in the same order, for a step whose obstacle stage ran as its own kernel the
 *      order of that kernel -- and NaN for a candidate without FX_FLAG_COSTED.  winner[v] is the lexicographic (total, index) minimum
 *      over the candidates with FX_FLAG_SELECTABLE and neither FX_FLAG_COLLISION nor FX_FLAG_BOUNDARY, NaN totals skipped: a LOCAL
 *      index in [0, C) as fx_read_ranked_agent answers them, also for a sharded agent; cost[v] its total.  Nothing eligible:
 *      winner[v] = -1, cost[v] = +inf.  totals, where not NULL, receives total(c) of every candidate, [n_vec][C].
 *      The call reads the raw cost rows and the flag plane of the step and writes a block of its own, allocated on the first call and
 *      grow-only; it launches on the context's stream and waits.  It is the device selection only: no host road-boundary walk.
 *      Checked before anything is allocated, copied or launched: FX_ERR_NOT_READY before the first evaluated step, when the inputs
 *      were rewritten since it, and for a step without FX_MODE_WRITE_COSTMAP; FX_ERR_INVALID_ARGUMENT for NULL ctx, w, winner or cost,
 *      an agent out of range, n_vec < 1 and a weight that is zero or not finite (cost_function.py:55-60 registers only non-zero
 *      weights: a zero weight is another cost list, whose summation form the step decides; negative weights are legal);
 *      FX_ERR_CAPACITY above 32 768 vectors per call. */
int32_t fx_rescore_agent(FxContext *ctx, int32_t agent, int32_t n_vec, const double *w /*[n_vec][n_cost]*/, int64_t *winner /*[n_vec]*/,
                         double *cost /*[n_vec]*/, double *totals /*[n_vec][C] or NULL*/);
/* fx_rescore_agent over the agent's EFFECTIVE cost list: the step's own list with up to two rows from outside
 * the step, as a cost that is partly summed beside the step has them.  pred [C], where not NULL, stands in place of the step's
 * prediction row (the prob of fx_eval_prediction_prob_agent, say); FX_ERR_INVALID_ARGUMENT for a list without FX_COST_PREDICTION.
 * resp [C], where not NULL, is ONE MORE term, where fx_eval_responsibility_cost_agent sums it: in front of the first entry whose id
 * is above FX_COST_PREDICTION, else at the end.  A weight vector then has n_eff = n_cost (+ 1 with resp) weights in that order, and
 * total(c) is the same sum over the effective list -- for a step whose obstacle stage ran as its own kernel the inserted term joins
 * the addend of the terms behind the prediction.  A NaN in either row is a NaN total, skipped like any other.  Everything else --
 * eligibility, ties, -1 / +inf, local indices, refusals, the block -- is fx_rescore_agent's; with both rows NULL so is every bit. */
int32_t fx_rescore_agent_rows(FxContext *ctx, int32_t agent, int32_t n_vec, const double *w /*[n_vec][n_eff]*/,
                              const double *pred /*[C] or NULL*/, const double *resp /*[C] or NULL*/, int64_t *winner /*[n_vec]*/,
                              double *cost /*[n_vec]*/, double *totals /*[n_vec][C] or NULL*/);
/* fx_rescore_agent_rows for n_agents agents of the context in one call: three launches at most, one copy up, one back, whatever the
 * number of agents, and for every agent the bits of its own call.  agents [n_agents] (NULL: 0 .. n_agents - 1) in any order;
 * n_vec [n_agents] vectors per listed agent; w the agents' [n_vec[i]][n_eff_i] weights one behind the other; pred / resp
 * [n_agents] pointers to rows [C_i], any of them NULL, or NULL for none; winner / cost the agents' [n_vec[i]] answers one behind
 * the other.  No totals.  Refused before anything is allocated, copied or launched, naming the agent: what fx_rescore_agent_rows
 * refuses for it, an agent out of range or listed twice (FX_ERR_INVALID_ARGUMENT), more than 32 768 vectors for one agent or a
 * flat grid above 2^31 - 1 workgroups (FX_ERR_CAPACITY).  n_agents == 0 returns FX_OK and touches nothing. */
int32_t fx_rescore_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents, const int32_t *n_vec, const double *w,
                         const double *const *pred, const double *const *resp, int64_t *winner, double *cost);
/* device time of the context's last re-score (events around its launches), ms; -1 before the first.  Waits for it. */
double fx_last_rescore_ms(FxContext *ctx);
/* device pointer of one agent's raw cost rows, f64 [n_cost][ld] -- the cost-map counterpart of fx_device_views.  FX_ERR_NOT_READY for a
 * step that stored no cost map (FX_MODE_WRITE_COSTMAP).  Any pointer may be NULL. */
int32_t fx_device_costmap_view(FxContext *ctx, int32_t agent, void **costmap, int64_t *ld, int32_t *n_cost);

/* ---- a finished plan step re-evaluated under many prediction sets at once, beside the step -- DESIGN.md section 25; additive
 *      within ABI 15 ----
 *      The walk of a step does not read the predictions; its obstacle stage -- the `prediction` cost and the collision walk -- reads
 *      only x, y, theta, the flag words and the obstacle tables.  One call answers, for n_hyp hypotheses, what a plan step with those
 *      predictions would have selected.  A hypothesis is the five obstacle arrays of FxStateUpdate WITH THE K AND P OF THE UPLOAD,
 *      exactly what fx_update_state accepts; an absent obstacle has obs_npred = 0 and obs_nhull = 0.  Everything else is the step's:
 *      ego state, sampling, cost list and weights, dto_pos, lanelets, hot_origin.
 *      The rule.  Let CH be the steps per item the obstacle kernel has, or would have, for this step (fx_step_info_ex's split_CH; a forced
 *      fx_set_obstacle_stage(.., steps_per_item) is honoured).  pred[h][c] is the raw prediction entry fx_obstacle_kernel would store;
 *      collision[h][c] the collision decision on the hypothesis' hulls; total[h][c] the weighted sum of the step's raw cost rows with
 *      pred[h][c] in the prediction entry, in the order of a step whose obstacle stage ran as its own kernel (NaN without
 *      FX_FLAG_COSTED; a list without FX_COST_PREDICTION sums as the step did); winner[h] the lexicographic (total, index) minimum
 *      over the candidates with FX_FLAG_SELECTABLE, without collision[h][c] and without FX_FLAG_BOUNDARY, NaN totals skipped -- a
 *      LOCAL index, -1 with cost +inf where nothing is eligible; n_collisions[h] the selectable colliding candidates ordered before
 *      the winner by (total, index), all of them where nothing is eligible.
 *      For a step whose obstacle stage ran in its own kernel the step's own arrays reproduce the step bit for bit, and any
 *      hypothesis equals a real step run with those arrays.  For a step that ran the stage INSIDE the walk the answer is, bit for
 *      bit, that of the same step forced to fx_set_obstacle_stage(ctx, 2, CH); against the fused step's own cost it agrees only up
 *      to the association of at most S - 1 non-negative addends -- the walk's lane-split associations are not emulated.
 *      It is the device selection only: no host road-boundary walk, no occlusion walk.  Synchronous; any agent of a batch context.
 *      The call packs one table per hypothesis into one staging buffer, copies it up once, enqueues at most three launches per
 *      round of hypotheses and copies the answers back; its block is allocated on first use, grow-only, counted in fx_device_bytes.
 *      Checked before anything is allocated, copied or enqueued: FX_ERR_NOT_READY before the first finished step, when the inputs
 *      were rewritten since it, and for a step without FX_MODE_WRITE_BUNDLE or without FX_MODE_WRITE_COSTMAP;
 *      FX_ERR_INVALID_ARGUMENT for n_hyp < 1, a NULL array in a hypothesis, NULL out, winner or cost, an agent out of range, an
 *      upload with K = 0, and a step the obstacle kernel does not serve (needs K <= 64, no road boundary, no windowed cost term);
 *      FX_ERR_CAPACITY above FX_HYPOTHESES_MAX hypotheses per call. */
#define FX_HYPOTHESES_MAX 4096
typedef struct FxHypothesis {
    const double *obs_pos;       /* [K][P][2] */
    const double *obs_cov_inv;   /* [K][P][4] */
    const int32_t *obs_npred;    /* [K] */
    const double *obs_hull;      /* [K][P-1][6] */
    const int32_t *obs_nhull;    /* [K] */
} FxHypothesis;
typedef struct FxHypothesisOutputs {
    int64_t *winner;         /* [n_hyp] */
    double *cost;            /* [n_hyp] */
    int64_t *n_collisions;   /* [n_hyp] or NULL */
    double *pred;            /* [n_hyp][C] or NULL: 0 without FX_FLAG_COSTED, as the step's cost map */
    double *total;           /* [n_hyp][C] or NULL */
    uint8_t *collision;      /* [n_hyp][C] or NULL */
} FxHypothesisOutputs;
int32_t fx_eval_hypotheses_agent(FxContext *ctx, int32_t agent, int32_t n_hyp, const FxHypothesis *hyp /*[n_hyp]*/,
                                 const FxHypothesisOutputs *out);
/* fx_eval_hypotheses_agent for n_agents agents of the context in one call: three launches per round, one copy
 * up, one back, whatever the number of agents, and for every listed agent every output bit for bit what fx_eval_hypotheses_agent
 * returns for that agent with those hypotheses on the same resident step.  agents [n_agents] (NULL: 0 .. n_agents - 1) in any order;
 * n_hyp [n_agents] hypotheses per listed agent; hyp the agents' [n_hyp[i]] hypotheses one behind the other, each with the K and P of
 * its agent's upload.  out->winner, cost and n_collisions hold the agents' [n_hyp[i]] answers one behind the other, in call order;
 * out->pred, total and collision, where not NULL, the agents' [n_hyp[i]][C_i] blocks one behind the other.  Every agent keeps the C,
 * ld, S, K and P of its own slot; all use the context's steps per item (split_CH), which the per-agent call reads.  A round takes
 * (agent, hypothesis) pairs in call order while its tables and scratch fit and no launch exceeds 2^31 - 1 workgroups; an agent's
 * hypotheses may be cut across rounds.  The block is the per-agent call's.
 * Refused before anything is allocated, copied or launched, naming the agent, the context left usable and fx_last_hypotheses_info
 * as it was: what fx_eval_hypotheses_agent refuses for it (n_hyp[i] < 1 included), an agent out of range or listed twice, NULL
 * n_hyp, hyp, out, winner or cost (FX_ERR_INVALID_ARGUMENT), more than FX_HYPOTHESES_MAX hypotheses for one agent or one hypothesis
 * of one agent whose items exceed 2^31 - 1 workgroups (FX_ERR_CAPACITY).  n_agents == 0 returns FX_OK and touches nothing. */
int32_t fx_eval_hypotheses_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /*[n_agents], NULL: 0 .. n_agents-1*/,
                                 const int32_t *n_hyp /*[n_agents]*/, const FxHypothesis *hyp /*the agents' [n_hyp[i]] one behind the other*/,
                                 const FxHypothesisOutputs *out);
/* device time of the context's last hypotheses call of either kind (events around its launches), ms; -1 before the first.  Waits
 * for it. */
double fx_last_hypotheses_ms(FxContext *ctx);
/* the last call's (of either kind) steps per item (CH), rounds of hypotheses and kernel launches; any pointer may be NULL.
 * FX_ERR_NOT_READY before the first call. */
int32_t fx_last_hypotheses_info(FxContext *ctx, int32_t *steps_per_item, int32_t *rounds, int32_t *launches);

/* ---- road boundary (replaces create_road_boundary_obstacle + trajectories_collision_static_obstacles,
 *      planner.py:362-381,550-565; commonroad-drivability-checker, not in the reference tree) ----
 * fx_build_boundary_bins: host-side geometry, no GPU.  Splits the n_seg boundary segments seg[n_seg][4] =
 * (ax, ay, bx, by) into pieces no longer than max_len, and lists for every reference knot k the pieces whose
 * midpoint lies within reach + half length of knot k.  piece_out[piece_cap][4], bin_out[M + 1],
 * item_out[item_cap]; *n_piece / *n_item receive the counts (FX_ERR_CAPACITY when a buffer is too small; the
 * counts are still set so the caller can re-allocate).  reach must cover the ego footprint around its foot point:
 * longest reference segment + largest |d| + wb_rear_axle + half diagonal of the vehicle. */
int32_t fx_build_boundary_bins(int32_t M, const double *ref_x, const double *ref_y, int32_t n_seg, const double *seg,
                               double max_len, double reach, int32_t piece_cap, double *piece_out, int32_t *n_piece,
                               int32_t *bin_out, int32_t item_cap, int32_t *item_out, int32_t *n_item);
/* first step at which each candidate's footprint meets the boundary, -1 if never (FX_MODE_ROAD_BOUNDARY);
 * boundary_harm = logistic regression of cartesian.v at that step (planner.py:369-375) is left to the caller */
int32_t fx_read_boundary_steps(FxContext *ctx, int32_t *steps);
int32_t fx_read_boundary_steps_agent(FxContext *ctx, int32_t agent, int32_t *steps);

/* device pointers of one agent's outputs for callers that keep working on the GPU:
 * cost f64[ld], flags u32[ld], planes f64[14][S][ld] (NULL without FX_MODE_WRITE_BUNDLE) */
int32_t fx_device_views(FxContext *ctx, int32_t agent, void **cost, void **flags, void **planes, int64_t *ld);

/* ---- measurement hooks (bench.py): device bytes owned; HIP-event time of the last step's device work
 *      (evaluation + selection kernels) and of the evaluation kernel alone ---- */
int64_t fx_device_bytes(const FxContext *ctx);
double fx_last_kernel_ms(const FxContext *ctx);
double fx_last_eval_kernel_ms(const FxContext *ctx);
/* selection fused into the evaluation kernel (default on): the evaluation kernel's last workgroup of an agent reduces the
 * partial arg-mins and publishes the result, so a plan step is a single launch.  With FX_MODE_COLLISION it also counts the
 * colliding candidates in front of the winner (planner.py:336-357) -- for agents of at most 8 192 candidates whose obstacle
 * stage runs inside the evaluation kernel (planner-sized steps; larger ones and steps whose obstacle stage is its own kernel keep
 * fx_select_kernel) -- and with fx_set_package it gathers the winner package: ReactivePlanner.plan() at the reference's operating
 * point (planning.yaml:34-35, 630 / 800 candidates) is ONE launch.  0 = always run the separate selection kernel (same results;
 * used by the parity tests), 1 = automatic, 2 = in-kernel whatever the candidate count (tests).  Takes effect at the next upload. */
int32_t fx_set_fused_selection(FxContext *ctx, int32_t enabled);
/* The whole plan step in ONE launch (csrc/fx_step_kernel.h; ABI 9), OPT-IN: steps whose obstacle stage runs as its own kernel
 * behind the walk (200 ... 3 072 waves with a materialised bundle: BASELINE config 3, config 4's batch) can run walk | grid barrier |
 * obstacle items | grid barrier | sliced selection (+ winner package) as phases of one kernel.  Same results (bit for bit at three
 * steps per item).  Measured slower on the MI355X -- config 3: 94 us against 86 us -- because the obstacle phase then runs with the
 * walk's register allocation (3 072 waves for ~5 000 work items: every wave runs two items' latency chains back to back), so it is off unless asked
 * for.  Needs every workgroup of the launch resident at once: the library sizes the launch by the occupancy query and keeps the three
 * launches where the walk alone would not fit.  The query assumes the device to itself: two such launches at a time (two contexts, two
 * processes) can hold each other's slots until the in-kernel barrier gives up after 2 s and the step ends in FX_ERR_TIMEOUT -- use it
 * from ONE context per device.  mode 0 / 1 = off (three launches), 2 = on where applicable (FX_STEP_KERNEL=1 in
 * the environment does the same for every context); steps_per_item 0 = automatic, or 3 / 5 / 8 steps of the horizon per obstacle
 * work item.  Takes effect at the next upload.  fx_step_info_ex [15] bit 16 reports that the last step ran this way. */
int32_t fx_set_step_kernel(FxContext *ctx, int32_t mode, int32_t steps_per_item);
/* how the last evaluation was launched: grid kernel, lanes per candidate, waves per SIMD, workgroup size, wave split, fused
 * selection, workgroups per agent, agents, winner package, dynamic LDS bytes */
int32_t fx_step_info(const FxContext *ctx, int64_t *out10);
/* the same ten values, then: [10] obstacle stage ran as its own kernel, [11] its steps per work item, [12] work items (waves) per
 * agent (max), [13] dynamic LDS bytes, [14] waves per workgroup when the chunks of a tile share one workgroup (0: one wave per
 * (tile, chunk) item), [15] what the agent's last workgroup did beyond the arg-min: bit 0 counted the collisions in front of the
 * winner, bit 1 gathered the winner package (0 with a separate selection kernel); bits 8-9 how the latest inputs (upload or state
 * update) reached the device: 1 DMA copy, 2 staging kernel reading the pinned block, 3 written by the host straight into device
 * memory -- where the device memory is mapped into the process (large BAR; probed at fx_create without risking a fault) a state
 * update needs no staging launch: posted writes, ordered in front of the evaluation launch.  FX_STAGE=kernel|dma|bar forces a path */
int32_t fx_step_info_ex(const FxContext *ctx, int64_t *out16);
/* HIP-event time of the obstacle kernel of the latest timed step / of the most recent <= max_n timed steps (FX_TIMING_KERNEL;
 * 0 where the stage ran fused into the walk) */
double fx_last_obstacle_kernel_ms(const FxContext *ctx);
int32_t fx_read_obstacle_kernel_times(FxContext *ctx, int32_t max_n, double *obst_ms, int32_t *n_out);
/* per-step HIP-event timing (default FX_TIMING_OFF: fx_finish only polls the result block the kernel publishes
 * into pinned host memory).  FX_TIMING_STREAM -- stream events around the kernels (the evaluation figure includes
 * the dispatch gap in front of the kernel); FX_TIMING_KERNEL -- start/stop events attached to the evaluation
 * kernel itself (hipExtLaunchKernel): the figure a kernel trace reports, at a few microseconds more host time per
 * timed launch.  Events live in a ring of 256 steps and are read on request only: fx_last_*_ms (latest timed
 * step) and fx_read_kernel_times (the most recent <= max_n timed steps, oldest first; n_out = how many) wait for
 * the events they read, fx_finish never does.  fx_set_timing_interval: time every n-th step only. */
enum { FX_TIMING_OFF = 0, FX_TIMING_STREAM = 1, FX_TIMING_KERNEL = 2 };
int32_t fx_set_timing(FxContext *ctx, int32_t mode);
int32_t fx_set_timing_interval(FxContext *ctx, int32_t every);
int32_t fx_read_kernel_times(FxContext *ctx, int32_t max_n, double *eval_ms, double *step_ms, int32_t *n_out);
/* device self-test of the kernel's elementary functions (atan, sin, cos) on n host values */
int32_t fx_math_selftest(int32_t n, const double *x, double *atan_out, double *sin_out, double *cos_out);
/* device self-test of ONE arithmetic primitive of the kernels (csrc/fx_math.h, fx_walk.h, fx_eval_kernel.h), elementwise over n
 * host elements, synchronous: allocates, copies, launches, synchronises, copies back and frees.  in[k] holds n elements of the
 * op's k-th operand, out[k] receives n doubles of its k-th result (entries beyond what the op uses are not read):
 *   ATAN, ATAN_TAB, ATAN_SMALL, ATAN_SMALL_TAB, RCP_NR, RCP_PRED, NP_ROUND5, WRAP_PM_2PI   in: x            out: f(x)
 *   SINCOS, SINCOS_TAB                                                                      in: x            out: sin, cos
 *   SQRT_RSQRT                                                                              in: x            out: sqrt, 1/sqrt
 *   FDIV (n / d), DIV_RCP (a / b with the reciprocal of rcp_nr)                             in: n, d         out: quotient
 *   OBB_HULL     in: [n][4] (c0x, c0y, u0x, u0y), [n][4] (c1x, c1y, u1x, u1y), [n][2] (hl, hw)              out: cx, cy, ex, ey, h1, h2
 *   OBB_OVERLAP  in: [n][6], [n][6] stored boxes (cx, cy, ex, ey, h1, h2)                                   out: 1.0 overlap, 0.0 separated
 * 1 <= n <= FX_SELFTEST_MAX_N.  WRAP_PM_2PI is a loop over |x| / 2 pi rounds: an input that is not finite or beyond
 * FX_SELFTEST_WRAP_MAX is refused (FX_ERR_INVALID_ARGUMENT) before anything is launched. */
enum {
    FX_SELFTEST_ATAN = 0, FX_SELFTEST_ATAN_TAB = 1, FX_SELFTEST_ATAN_SMALL = 2, FX_SELFTEST_ATAN_SMALL_TAB = 3,
    FX_SELFTEST_SINCOS = 4, FX_SELFTEST_SINCOS_TAB = 5, FX_SELFTEST_RCP_NR = 6, FX_SELFTEST_RCP_PRED = 7, FX_SELFTEST_FDIV = 8,
    FX_SELFTEST_SQRT_RSQRT = 9, FX_SELFTEST_DIV_RCP = 10, FX_SELFTEST_NP_ROUND5 = 11, FX_SELFTEST_WRAP_PM_2PI = 12,
    FX_SELFTEST_OBB_HULL = 13, FX_SELFTEST_OBB_OVERLAP = 14, FX_SELFTEST_N_OPS = 15
};
#define FX_SELFTEST_MAX_N (1 << 22)
#define FX_SELFTEST_WRAP_MAX 100.0
int32_t fx_device_selftest(int32_t op, int32_t n, const double *const *in, double *const *out);

/* ---- trajectory risk: collision probability x harm (risk_costs.py:20-118, crash_angle_simplified) -- DESIGN.md section 11 ----
 * Nothing here runs unless called: the plan step, its launches and its buffers are unchanged.  The risk buffers are allocated
 * on the first fx_eval_risk_agent. */
enum { FX_RISK_PROB_MVN = 0, FX_RISK_PROB_MAHALANOBIS = 1 };            /* risk.json fast_prob_mahalanobis false / true */
enum { FX_RISK_HARM_LOGISTIC = 0, FX_RISK_HARM_REF_SPEED = 1 };          /* model of a protected pair / of the ego vs. unprotected */
enum { FX_RISK_CLASS_UNPROTECTED = 0, FX_RISK_CLASS_PROTECTED = 1 };     /* harm_estimation.py obstacle_protection */
#define FX_RISK_MAX_EDGES 6
typedef struct FxRiskParams {
    int32_t prob_mode;       /* FX_RISK_PROB_* */
    int32_t prot_model;      /* protected obstacle, ego and obstacle harm: FX_RISK_HARM_LOGISTIC 1/(1+exp(-c - s dv - bin(angle)))
                                or FX_RISK_HARM_REF_SPEED dv < ref ? (dv/ref)^exp : 1 (ignore_angle only) */
    int32_t unprot_ego_model;/* ego harm against an unprotected obstacle: FX_RISK_HARM_LOGISTIC (c, s) or FX_RISK_HARM_REF_SPEED */
    int32_t n_edges;         /* impact-area bins of the protected logistic model: 6 (12 areas), 2 (4 areas), 0 (angle ignored) */
    double edges[FX_RISK_MAX_EDGES];     /* ascending |angle| edges [rad]: (-e0, e0) is the front bin (coefficient 0) */
    double coef_pos[FX_RISK_MAX_EDGES];  /* [j], j >= 1: angle in [e(j-1), e(j)) */
    double coef_neg[FX_RISK_MAX_EDGES];  /* [j], j >= 1: angle in (-e(j), -e(j-1)] */
    double coef_else;                    /* every other angle (rear; NaN; angles are not wrapped) */
    double prot_c, prot_s;               /* protected logistic model: const, speed */
    double prot_ref, prot_exp;           /* protected reference-speed model */
    double uego_c, uego_s;               /* ego vs. unprotected, logistic: 1/(1+exp(-c - s dv)) */
    double uego_ref, uego_exp;           /* ego vs. unprotected, reference speed */
    double ped_c, ped_s;                 /* unprotected obstacle: 1/(1+exp(c - s dv)) */
    double ego_length, ego_width, ego_mass;
} FxRiskParams;
/* Predictions of the K obstacles, once per plan step: pos [K][P][2], cov [K][P][4] (raw), cov_inv [K][P][4] (Mahalanobis mode;
 * may be NULL otherwise), yaw [K][P], v [K][P]; n_pos [K] = len(pos_list) (<= P), n_yaw / n_v [K] the lengths of
 * orientation_list / v_list; length, width, mass [K]; cls [K] FX_RISK_CLASS_*.  Checked at fx_eval_risk_agent against the
 * step's horizon: yaw must cover min(S, n_pos) entries and v min(S - 1, n_pos) (collision_probability.py:180,
 * harm_estimation.py:282-300).  K = 0 clears. */
int32_t fx_set_risk_obstacles_agent(FxContext *ctx, int32_t agent, int32_t K, int32_t P, const double *pos, const double *cov,
                                    const double *cov_inv, const double *yaw, const double *v, const int32_t *n_pos,
                                    const int32_t *n_yaw, const int32_t *n_v, const double *length, const double *width,
                                    const double *mass, const int32_t *cls);
/* ego_risk / obst_risk of candidates of the last plan step (max over obstacles of max over steps of harm x probability) and the
 * arg-min of ego + obst over them, ties to the lower candidate index (-1 when there is none).  ids NULL: every candidate whose
 * flags hold VALID, FEASIBLE and RETURNED; ego_risk / obst_risk then have C entries, NaN for the others.  Otherwise the n_ids
 * listed candidates, in that order.  Needs FX_MODE_WRITE_BUNDLE (FX_ERR_NOT_READY otherwise) -- or, ABI 13, a non-NULL ids all of which
 * lie in the agent's sparse set (fx_materialise_candidates_agent): the pass then reads the set's rows, and the returned arg-min is a
 * candidate index as ever.  Synchronous. */
int32_t fx_eval_risk_agent(FxContext *ctx, int32_t agent, const FxRiskParams *params, int64_t n_ids, const int64_t *ids,
                           double *ego_risk, double *obst_risk, int64_t *min_risk_index);
/* device time of the last fx_eval_risk_agent (risk pass + arg-min) or fx_eval_risk_costs_agent (all its kernels), ms */
double fx_last_risk_ms(FxContext *ctx);

/* ---- per-obstacle risk and harm, risk-cost principles, responsibility (risk_costs.py:20-251, utility/responsibility.py) --
 *      DESIGN.md section 13; ABI 12.  Beside the plan step like the block above: nothing here runs unless called. ---- */
enum { FX_RISK_RESP_NONE = 0, FX_RISK_RESP_ACTION_SPACE = 1, FX_RISK_RESP_REACH_SET = 2 };   /* get_responsibility_cost mode */
enum { FX_RISK_BOUNDARY_ZERO = 0, FX_RISK_BOUNDARY_ARRAY = 1, FX_RISK_BOUNDARY_STEP = 2 };
typedef struct FxRiskCostParams {
    double weights[5];          /* total = sum w_i principle_i: bayes, equality, maximin, ego, responsibility */
    double maximin_eps;         /* get_maximin_costs eps (upstream 10e-10) */
    double maximin_scale;       /* ... and scale_factor (upstream 10) */
    int32_t boundary_mode;      /* FX_RISK_BOUNDARY_ZERO; _ARRAY: boundary_harm below; _STEP: 1/(1+exp(-c - s v[first step outside the
                                   road])) for candidates with FX_FLAG_BOUNDARY, 0 for the others and for a step that ran without
                                   FX_MODE_ROAD_BOUNDARY (planner.py:369-375) */
    int32_t responsibility_mode;/* FX_RISK_RESP_*; _REACH_SET reads the tables of fx_set_reach_sets_agent */
    double boundary_c, boundary_s;   /* harm_parameters.json log_reg.ignore_angle const / speed (_STEP) */
    const double *boundary_harm;     /* [n] (n = n_ids, or C with ids NULL), _ARRAY */
    const double *responsibility;    /* [K] 0 / 1 per obstacle (_ACTION_SPACE): 0 inside the ego's +-pi/4 view (check_if_inside180view) */
} FxRiskCostParams;
/* Every pointer may be NULL.  n = n_ids, or C with ids NULL (NaN rows for the candidates that are not selected).  The per-obstacle
 * results are obstacle-major, [K][n]: column k of candidate j at [k * n + j]. */
typedef struct FxRiskOutputs {
    double *ego_risk, *obst_risk;        /* [n] as fx_eval_risk_agent returns them, bit for bit */
    double *obst_harm_occ;               /* [n] max over obstacles of: obstacle harm at the first arg-max of the probability list if
                                            that maximum is > 0.001, else 0 */
    double *ego_risk_max, *obst_risk_max, *ego_harm_max, *obst_harm_max;   /* [K][n] maxima over t */
    double *bayes, *equality, *maximin, *ego, *responsibility, *total;     /* [n]; written with cost parameters only */
    double *boundary_harm;               /* [n] the boundary harm the principles used; with cost parameters only */
    int64_t *min_risk_index;             /* arg-min of ego_risk + obst_risk, as fx_eval_risk_agent */
    int64_t *min_cost_index;             /* arg-min of total: ties to the lower candidate index, NaN totals skipped, -1 when nothing
                                            is left or without cost parameters */
} FxRiskOutputs;
/* Reach sets of one agent for FX_RISK_RESP_REACH_SET (calc_responsibility_reach_set), after fx_set_risk_obstacles_agent (which
 * clears them): entry e is a reach-set obstacle, entry_obs [n_entries] its index among the K prediction obstacles, its parts
 * entry_part_off[e] .. entry_part_off[e + 1] (the host drops the parts with time_t <= 0); part p tests the ego point
 * (x, y)[part_step[p]] against the polygon verts[part_vert_off[p] .. part_vert_off[p + 1]][2] (>= 3 vertices; closing or padding a
 * ring with repeated vertices does not change the result): strict interior by the even-odd crossing rule.  The cost is
 * -sum obst_risk_max[entry_obs[e]] over the entries none of whose parts contains its point.  Indices are checked against K and the
 * horizon at fx_eval_risk_costs_agent.  n_entries = 0 clears. */
int32_t fx_set_reach_sets_agent(FxContext *ctx, int32_t agent, int32_t n_entries, const int32_t *entry_obs,
                                const int32_t *entry_part_off, int32_t n_parts, const int32_t *part_step,
                                const int32_t *part_vert_off, int32_t n_verts, const double *verts);
/* calc_risk's seven results for candidates of the last plan step and, with cost != NULL, the risk-cost principles and their
 * weighted total with its arg-min.  ids as in fx_eval_risk_agent.  An obstacle with min(S - 1, n_pos) == 0 is refused
 * (FX_ERR_INVALID_ARGUMENT: np.max of an empty list upstream).  Needs FX_MODE_WRITE_BUNDLE (FX_ERR_NOT_READY otherwise), or listed
 * candidates of the agent's sparse set as fx_eval_risk_agent does.
 * Synchronous; its buffers are allocated on first use and counted in fx_device_bytes; fx_last_risk_ms covers it. */
int32_t fx_eval_risk_costs_agent(FxContext *ctx, int32_t agent, const FxRiskParams *params, const FxRiskCostParams *cost /* NULL: detail only */,
                                 int64_t n_ids, const int64_t *ids, const FxRiskOutputs *out);

/* ---- Collision probability as the prediction cost (additive within ABI 14) ----
 * The `prediction` cost of the reference's C++ route, cf.CalculateCollisionProbabilityFast (reactive_planner_cpp.py:151-155):
 * Sum over the predictions, in their order, of Sum_i get_collision_probability_fast(...)[i] (collision_probability.py:141-261;
 * partial_cost_functions.py:344-356, the commented-out branch) for candidates of the last plan step, and the step's weighted cost
 * re-summed with that entry in place of the step's own.  A pass of its own beside the step: nothing a plan step, the top-k, a
 * sparse set, a sort or the risk passes own is written.  Obstacles: the tables of fx_set_risk_obstacles_agent, of which pos, cov,
 * yaw, n_pos, n_yaw and length are read.  wb_rear_axle of the functor is not used (UNPINNED: DESIGN.md section 16). */
enum { FX_PRED_SOURCE_PROBABILITY = 0,   /* the collision probability */
       FX_PRED_SOURCE_STEP = 1 };        /* the step's own raw prediction entry: no probability kernel runs and `total` is the
                                            step's cost bit for bit -- the self-check of summation order and weights */
typedef struct FxPredProbParams {
    double ego_length, ego_width;
    int32_t source;                      /* FX_PRED_SOURCE_* */
} FxPredProbParams;
typedef struct FxPredProbOutputs {       /* rows in the order of ids, or [C] with ids == NULL: NaN for candidates without
                                            FX_FLAG_COSTED, which the arg-min skips.  Any pointer may be NULL */
    double *prob;                        /* [n] raw cost Sum_k Sum_i p (FX_PRED_SOURCE_STEP: the step's raw prediction entry) */
    double *prob_obs;                    /* [K][n] per prediction, obstacle-major (FX_PRED_SOURCE_STEP: NaN) */
    double *total;                       /* [n] the weighted cost sum of the step's raw cost rows with the prediction entry replaced
                                            by prob, in the step's own order of operations */
    int64_t *best_index;                 /* lexicographic (total, index) minimum over the candidates with FX_FLAG_SELECTABLE and
                                            neither FX_FLAG_COLLISION nor FX_FLAG_BOUNDARY, NaN totals skipped; -1: none */
    double *best_cost;                   /* its total (NaN with -1) */
} FxPredProbOutputs;
/* ids as in fx_eval_risk_agent (n_ids == 0 with ids == NULL: every candidate).  Checked before anything is launched or written:
 * FX_ERR_NOT_READY before the first evaluated step or when inputs were rewritten since it, for a step without
 * FX_MODE_WRITE_COSTMAP, and without FX_MODE_WRITE_BUNDLE unless every listed id lies in the agent's sparse set;
 * FX_ERR_INVALID_ARGUMENT for a cost list without FX_COST_PREDICTION, NULL params or out, lengths that are not positive, an unknown
 * source, ids out of range, or an obstacle whose yaw is shorter than min(S, n_pos).  K = 0 is legal: prob = 0, total = the re-sum.
 * Synchronous; its part of the risk passes' device block is allocated on first use, only grows and is counted in fx_device_bytes. */
int32_t fx_eval_prediction_prob_agent(FxContext *ctx, int32_t agent, const FxPredProbParams *params, int64_t n_ids, const int64_t *ids,
                                      const FxPredProbOutputs *out);
/* device time of the last fx_eval_prediction_prob_agent or fx_eval_prediction_prob_batch (all its kernels), ms; -1 before the first */
double fx_last_predprob_ms(FxContext *ctx);

/* The same pass over EVERY candidate of several agents of the last plan step in one call (additive within
 * ABI 15): the ids == NULL form of fx_eval_prediction_prob_agent for each listed agent -- NaN rows for candidates without
 * FX_FLAG_COSTED, which the arg-min skips -- with the agent's own params[i], its own fx_set_risk_obstacles_agent tables, C, S, K and
 * cost list.  Every result is bit for bit what the per-agent call returns, whichever agents share a call.  Listed candidates,
 * sparse sets and prob_obs stay with the per-agent call. */
typedef struct FxPredProbBatchOutputs {  /* any pointer may be NULL */
    double *prob, *total;                /* [sum of C over the listed agents], agent-major: the rows of agents[i] start at the sum of
                                            C of agents[0..i) */
    int64_t *best_index;                 /* [n_agents], as FxPredProbOutputs.best_index (index within the agent's shard; -1: none) */
    double *best_cost;                   /* [n_agents] */
} FxPredProbBatchOutputs;
/* agents: n_agents distinct agents of the last upload in any order, or NULL: 0 .. n_agents - 1.  Everything is checked for every
 * listed agent before anything is launched, uploaded or written to out, and the message names the first offending agent:
 * FX_ERR_NOT_READY before the first evaluated step, when inputs were rewritten since it, and for an agent whose step ran without
 * FX_MODE_WRITE_COSTMAP or without FX_MODE_WRITE_BUNDLE; FX_ERR_INVALID_ARGUMENT for NULL ctx, params or out, n_agents < 0 or above
 * the uploaded agents, an agent out of range or listed twice, and per agent for what fx_eval_prediction_prob_agent refuses.
 * n_agents == 0 returns FX_OK and touches nothing.  Synchronous; fx_last_predprob_ms covers it; its memory is the risk passes'
 * device block (grow-only, counted in fx_device_bytes). */
int32_t fx_eval_prediction_prob_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /* NULL: 0 .. n_agents-1 */,
                                      const FxPredProbParams *params /* [n_agents] */, const FxPredProbBatchOutputs *out);

/* ---- The responsibility cost as a weighted term of the step's cost.  Beside the plan step like the
 *      blocks above: nothing here runs unless called. ----
 * ABI 15 removed the choice between two decompositions of the risk walk (a setter and its two constants), which changed no bit:
 * every risk pass -- fx_eval_risk_agent, fx_eval_risk_costs_agent and the call below -- evaluates the (obstacle, step) pairs of a
 * candidate with one wave per (tile of 64 candidates, chunk of steps, obstacle) and a finish kernel that combines the chunks.  The
 * partials of these items live in the risk passes' device block (at most 64 MiB of it where one candidate's share allows; the
 * candidates are batched).
 * responsibility (partial_cost_functions.py:359-387): get_responsibility_cost over calc_risk's obst_risk_max of a candidate, times
 * its weight, as one more term of the weighted cost sum at its place in the name-sorted list -- behind `prediction`, in front of
 * `velocity_offset`.  The term inside the total never ran upstream (UNPINNED: DESIGN.md section 17); its per-candidate value is the
 * `responsibility` of fx_eval_risk_costs_agent. */
typedef struct FxRespCostParams {
    double weight;                   /* cost_weights["responsibility"]: not 0, not NaN */
    int32_t responsibility_mode;     /* FX_RISK_RESP_ACTION_SPACE or FX_RISK_RESP_REACH_SET (the tables of fx_set_reach_sets_agent) */
    const double *responsibility;    /* [K] 0 / 1 per obstacle (_ACTION_SPACE), as in FxRiskCostParams */
    const double *prediction;        /* [n] raw prediction entry to sum instead of the step's own -- the prob of
                                        fx_eval_prediction_prob_agent over the same candidates -- or NULL: the step's own */
} FxRespCostParams;
typedef struct FxRespCostOutputs {   /* rows in the order of ids, or [C] with ids == NULL: NaN for candidates without
                                        FX_FLAG_COSTED, which the arg-min skips.  No pointer may be NULL */
    double *resp;                    /* [n] the raw responsibility cost */
    double *total;                   /* [n] the step's raw cost rows re-summed with weight * resp at its place, in the step's own
                                        order of operations (a step whose obstacle stage ran as its own kernel: the term joins the
                                        addend of the terms behind the prediction) */
    double *ego_risk, *obst_risk;    /* [n] as fx_eval_risk_agent returns them */
    int64_t *best_index;             /* as FxPredProbOutputs.best_index */
    double *best_cost;
} FxRespCostOutputs;
/* ids as in fx_eval_prediction_prob_agent.  Checked before anything is launched or written: FX_ERR_NOT_READY before the first
 * evaluated step or when inputs were rewritten since it, for a step without FX_MODE_WRITE_COSTMAP, and without
 * FX_MODE_WRITE_BUNDLE unless every listed id lies in the agent's sparse set; FX_ERR_INVALID_ARGUMENT for what
 * fx_eval_risk_costs_agent refuses (an obstacle with min(S - 1, n_pos) == 0 among it), a zero or NaN weight, another
 * responsibility_mode, a NULL params, resp, out or output pointer.  K = 0 is legal: resp = 0 and total is the step's cost.
 * Synchronous; fx_last_risk_ms covers it. */
int32_t fx_eval_responsibility_cost_agent(FxContext *ctx, int32_t agent, const FxRiskParams *params, const FxRespCostParams *resp,
                                          int64_t n_ids, const int64_t *ids, const FxRespCostOutputs *out);

/* The same pass over EVERY candidate of several agents of the last plan step in one call (additive within
 * ABI 15): the ids == NULL form of fx_eval_responsibility_cost_agent for each listed agent -- NaN rows for candidates without
 * FX_FLAG_COSTED -- with the agent's own params[i] and resp[i] (weight, mode, responsibility [K of that agent], prediction [C of
 * that agent] or NULL), its own fx_set_risk_obstacles_agent and fx_set_reach_sets_agent tables, C, S, K, cost list and deferred-sum
 * mode.  Every output is bit for bit what the per-agent call returns, whichever agents share a call and in whatever order. */
typedef struct FxRespCostBatchOutputs {      /* no pointer may be NULL */
    double *resp, *total, *ego_risk, *obst_risk;  /* [sum of C over the listed agents], agent-major, as FxPredProbBatchOutputs */
    int64_t *best_index;                          /* [n_agents], as FxRespCostOutputs.best_index */
    double *best_cost;                            /* [n_agents] */
} FxRespCostBatchOutputs;
/* agents: as in fx_eval_prediction_prob_batch.  Everything is checked for every listed agent before anything is launched, uploaded,
 * allocated or written to out, and the message names the first offending agent: FX_ERR_INVALID_ARGUMENT for NULL ctx, params, resp,
 * out or output pointer, n_agents < 0 or above the uploaded agents, an agent out of range or listed twice; per agent what
 * fx_eval_responsibility_cost_agent refuses, with its codes.  n_agents == 0 returns FX_OK and touches nothing.  Synchronous;
 * fx_last_risk_ms covers it; its memory is the risk passes' device block (grow-only, counted in fx_device_bytes). */
int32_t fx_eval_responsibility_cost_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /* NULL: 0 .. n_agents-1 */,
                                          const FxRiskParams *params /* [n_agents] */, const FxRespCostParams *resp /* [n_agents] */,
                                          const FxRespCostBatchOutputs *out);

/* ---- The risk of listed candidates for several agents in one call (additive within ABI 15) ----
 * fx_eval_risk_agent(ctx, agents[i], &params[i], n_ids[i], ids[i], ...) for each listed agent: an agent with a list gets the
 * n_ids[i] listed candidates in that order, evaluated whatever their flags; an agent without one (ids[i] NULL with n_ids[i] == 0,
 * or n_ids NULL: no agent has a list) every candidate, NaN rows for those that lack VALID, FEASIBLE or RETURNED.  An agent whose
 * step stored no bundle takes part with a list inside its sparse set (fx_materialise_candidates_agent), as in the per-agent call.
 * Every output is bit for bit what the per-agent call returns, whichever agents and forms share a call and in whatever order.  The
 * detail and cost passes of a batch: fx_eval_risk_costs_batch below. */
typedef struct FxRiskBatchOutputs {      /* no pointer may be NULL */
    double *ego_risk, *obst_risk;        /* [sum of n_a], agent-major; n_a = n_ids[i], or C of the agent without a list */
    int64_t *min_risk_index;             /* [n_agents], as fx_eval_risk_agent's: a candidate index, ties to the lower candidate
                                            index whatever the list's order; -1: none */
} FxRiskBatchOutputs;
/* agents: as in fx_eval_prediction_prob_batch.  Everything is checked for every listed agent before anything is launched, uploaded,
 * allocated or written to out, and the message names the first offending agent: FX_ERR_INVALID_ARGUMENT for NULL ctx, params, out
 * or output pointer, n_agents < 0 or above the uploaded agents, an agent out of range or listed twice, n_ids[i] > 0 with ids[i]
 * NULL; per agent what fx_eval_risk_agent refuses, with its codes (a step without FX_MODE_WRITE_BUNDLE and an id outside the sparse
 * set: FX_ERR_NOT_READY).  Unlike the per-agent call, the batch also refuses (FX_ERR_NOT_READY) inputs rewritten since the last
 * evaluation (fx_update_state): it is made behind a plan step of all its agents.  n_agents == 0 returns FX_OK and touches nothing.
 * Synchronous; fx_last_risk_ms covers it; its memory is the risk passes' device block (grow-only, counted in fx_device_bytes). */
int32_t fx_eval_risk_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /* NULL: 0 .. n_agents-1 */,
                           const FxRiskParams *params /* [n_agents] */,
                           const int64_t *n_ids /* [n_agents], or NULL: no agent has a list */,
                           const int64_t *const *ids /* [n_agents], ids[i] NULL with n_ids[i] == 0: every candidate */,
                           const FxRiskBatchOutputs *out);

/* ---- Risk detail and risk costs for several agents in one call (additive within ABI 15) ----
 * fx_eval_risk_costs_agent(ctx, agents[i], &params[i], cost[i], n_ids[i], ids[i], ...) for each listed agent, each with its own
 * obstacle and reach-set tables, its own list or none (as in fx_eval_risk_batch: n_a = n_ids[i], or C without a list) and its own
 * FxRiskCostParams or none -- weights, boundary mode, boundary_harm [n_a], responsibility [K_a], responsibility mode.  An agent
 * whose step stored no bundle takes part with a list inside its sparse set, as in the per-agent call.  Every output is bit for bit
 * what the per-agent call returns, whichever agents and forms share a call and in whatever order. */
typedef struct FxRiskCostBatchOutputs {   /* any pointer may be NULL, as in FxRiskOutputs */
    double *ego_risk, *obst_risk, *obst_harm_occ;                        /* [sum of n_a], agent-major */
    double *ego_risk_max, *obst_risk_max, *ego_harm_max, *obst_harm_max; /* agent i: [K_i][n_i] at offset sum_{b<i} K_b n_b */
    double *bayes, *equality, *maximin, *ego, *responsibility, *total, *boundary_harm;   /* [sum of n_a]; rows of an agent
                                                                            without cost parameters are left unwritten */
    int64_t *min_risk_index;   /* [n_agents] */
    int64_t *min_cost_index;   /* [n_agents]; -1 for an agent without cost parameters */
} FxRiskCostBatchOutputs;
/* agents: as in fx_eval_prediction_prob_batch.  Everything is checked for every listed agent before anything is launched, uploaded,
 * allocated or written to out, and the message names the first offending agent: FX_ERR_INVALID_ARGUMENT for NULL ctx, params or
 * out, n_agents < 0 or above the uploaded agents, an agent out of range or listed twice, n_ids[i] > 0 with ids[i] NULL; per agent
 * what fx_eval_risk_costs_agent refuses, with its codes (an obstacle with min(S - 1, n_pos) == 0, the reach-set and cost-mode
 * checks; a step without FX_MODE_WRITE_BUNDLE and an id outside the sparse set: FX_ERR_NOT_READY).  Like fx_eval_risk_batch it
 * also refuses (FX_ERR_NOT_READY) inputs rewritten since the last evaluation (fx_update_state).  n_agents == 0 returns FX_OK and
 * touches nothing.  Synchronous; fx_last_risk_ms covers it; its memory is the risk passes' device block (grow-only, counted in
 * fx_device_bytes). */
int32_t fx_eval_risk_costs_batch(FxContext *ctx, int32_t n_agents, const int32_t *agents /* NULL: 0 .. n_agents-1 */,
                                 const FxRiskParams *params /* [n_agents] */,
                                 const FxRiskCostParams *const *cost /* [n_agents], entry NULL: detail only; or NULL: all detail only */,
                                 const int64_t *n_ids /* [n_agents] or NULL */, const int64_t *const *ids,
                                 const FxRiskCostBatchOutputs *out);

#ifdef __cplusplus
}
#endif
#endif /* FXPLAN_H */
