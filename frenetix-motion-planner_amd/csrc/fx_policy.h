// fx_policy.h -- the launch policy of the plan step as pure functions of their arguments: no HIP runtime call, no environment, no
// allocation (tests/test_launch_policy.py runs them without a GPU, tests/policy_table.cpp).
//   fx_plan_upload       what an upload decides: work decomposition, kernels, LDS, the agents' places in the context's arrays
//   fx_plan_launches     what an evaluation decides: which kernels follow the walk and who ends the step
//   fx_plan_step_kernel  the one-launch step's (steps per item, workgroups, LDS) from the device's occupancy answers
// Problems are taken as validated (fx_context.h, validate()).
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include "fx_device.h"

// everything a caller (fx_set_*) or an experiment (environment) can force; 0 = automatic
struct FxForce {
    int G = 0, wpe = 0;            // fx_set_tuning: lanes per candidate, waves per SIMD
    int variant = 0;               // 0 auto, 1 generic kernel, 2 grid kernel
    int block = 0;                 // grid-kernel workgroup size (fx_set_block_size)
    int wsplit = 0;                // 0 auto, 1 lane split, 2 wave split (fx_set_part_mapping)
    int obst_stage = 0;            // obstacle stage: 0 auto, 1 fused into the walk, 2 its own kernel (fx_set_obstacle_stage; FX_OBST_STAGE)
    int obst_CH = 0;               // steps per work item of the obstacle kernel
    int step_kernel = 0;           // the whole step in ONE launch: 0 / 1 off, 2 on where applicable (fx_set_step_kernel; FX_STEP_KERNEL=0/1)
    int step_kernel_CH = 0;        // steps per obstacle item in that kernel (3, 5 or 8)
    int store = 0;                 // 0 auto, 1 write-back, 2 write-through plane stores (fx_set_store_mode)
    bool fuse_enabled = true;      // fx_set_fused_selection
    bool fuse_any_size = false;    // ... (ctx, 2): no candidate bound on the in-kernel collision count
    // experiments (environment)
    size_t lds_pad = 0;            // FX_LDS_PAD: occupancy cap through LDS
    int64_t tail_max_c = 8192;     // FX_TAIL_MAX_C: candidates per agent up to which the step's last workgroup counts the collisions (fx_plan_upload)
    int obst_wg = 0;               // FX_OBST_WG: 1 single-wave items, 2 workgroups
    bool obst_chunk_index = false; // FX_OBST_CHUNK_INDEX=1: the obstacle workgroup's waves take their chunks by index (FX_MODE_INT_CHUNK_INDEX)
};

// the context's capacities (fx_create_batch)
struct FxCaps {
    int64_t max_cand = 0, total_ld = 0, max_blocks_total = 0;
    int32_t max_steps = 0, max_knots = 0, max_obs = 0, max_pred = 0;
};
inline FxCaps fx_caps_of(int32_t max_agents, int64_t max_cand, int32_t max_steps, int32_t max_knots, int32_t max_obs, int32_t max_pred) {
    FxCaps k;
    k.max_cand = max_cand; k.max_steps = max_steps; k.max_knots = max_knots; k.max_obs = max_obs; k.max_pred = std::max(max_pred, 2);
    k.total_ld = (max_cand + 63) / 64 * 64 + 64 * (int64_t)max_agents;   // every agent's leading dimension is rounded up to 64 candidates
    k.max_blocks_total = k.total_ld / 2 + max_agents + 1;                // 64-lane workgroups at G = 32: 2 candidates each
    return k;
}

struct FxAgentPlan {
    int64_t C = 0, g_base = 0, ld = 0;
    int64_t cand_off = 0, block_off = 0;   // the agent's place in the per-candidate / per-workgroup arrays
    int32_t walk_blocks = 0, n_blocks = 0; // workgroups of the walk; arg-min partials (tiles where the obstacle kernel writes them)
    bool deferred = false;                 // the obstacle kernel runs this agent's obstacle stage
    uint32_t mode = 0;                     // DevProblem.mode: the problem's, minus stages without inputs, plus FX_MODE_INT_*
    size_t planes_off = 0;                 // bytes into the planes
    size_t obs_part_off = 0, obs_colm_off = 0, obs_tick_off = 0;   // elements into the obstacle kernel's scratch
};

struct FxStepPlan {
    int n_agents = 0;
    int G = 1, wpe = 2;                    // lanes per candidate / occupancy target
    bool use_grid = false;                 // fx_eval_grid_kernel
    int block = FX_BLOCK;
    size_t lds = 0;
    bool wsplit = false;
    bool split = false;                    // fx_obstacle_kernel behind the walk
    int split_CH = 3;
    size_t obs_lds = 0;                    // one item's staging area in that kernel
    size_t gen_rec_lds = 0;                // generic kernel, >= 4 lanes per candidate: bytes of the staged obstacle records + step masks
    bool any_bundle = false, any_obst = false, any_extra = false;
    bool count = false;                    // some agent runs the collision stage inside the evaluation kernel
    bool fusable = false, wt = false, step_kernel_ok = false;
    int M_max = 0, K_max = 0, S_max = 0;
    int64_t C_max = 0;
    int max_blocks = 0;                    // workgroups of the walk per agent (max)
    int obs_blocks = 0, obs_tiles = 0, obs_wg_waves = 0;   // obstacle kernel: items, tiles, chunks of the horizon per agent (max)
    size_t planes_bytes = 0, obs_part_n = 0, obs_colm_n = 0, obs_tick_n = 0;   // what the step needs of the grown buffers
    FxAgentPlan *agents = nullptr;         // [n_agents], the caller's storage
};

// what one evaluation launches (rebuilt by every fx_evaluate)
struct FxLaunchPlan {
    bool eval_launched = false;
    bool fused = false;                    // the evaluation kernel's last workgroup selects and publishes
    bool pkg = false;                      // the step gathers a winner package
    uint32_t tail = 0;                     // FX_TAIL_*: what that workgroup does beyond the arg-min
    bool try_step_kernel = false;          // the one-launch step comes first where the device holds it (fx_plan_step_kernel)
    bool obstacle = false;                 // fx_obstacle_kernel runs
    int obs_wg = 0;                        // ... its waves per workgroup (0: single-wave items)
    size_t obs_lds = 0;
    bool select = false, package = false;  // the selection / the package kernel follows
    bool one_launch = false;               // the evaluation kernel is the whole step
    // the one-launch step, when it ran: workgroups per agent, steps per item, LDS
    bool step_kernel = false;
    int step_blocks = 0, step_CH = 0;
    size_t step_lds = 0;
};

struct FxStepKernelSize {
    int CH = 0, blocks = 0;                // CH = 0: three launches
    size_t lds = 0;
};

inline int fx_policy_err(char *err, size_t err_len, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, err_len, fmt, ap);
    va_end(ap);
    return code;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// bundles up to this size use write-through plane stores.  tools/store_sweep.py on MI355X: write-through is faster up to
// ~0.5 GB (41 vs 45 us at 175 MB) and equal beyond (740 vs 746 us at 3.5 GB), so there is no upper limit by default.
#define FX_STORE_WT_MAX_BYTES (~(size_t)0)

// ---- the rules, each written once ----
// windowed (Simpson) costs need the whole horizon in one lane and the generic kernel
inline bool fx_is_windowed_cost(int id) {
    const unsigned windowed = 1u << FX_COST_ACCELERATION | 1u << FX_COST_JERK | 1u << FX_COST_ORIENTATION_OFFSET | 1u << FX_COST_PATH_LENGTH |
                              1u << FX_COST_DISTANCE_TO_OBSTACLES | 1u << FX_COST_LANE_CENTER_OFFSET;
    return (windowed >> id) & 1u;   // (ids are validated: 0 <= id < FX_NUM_COSTS)
}
inline bool fx_has_windowed_cost(const FxProblem *p) {
    bool extra = false;
    for (int n = 0; n < p->n_cost; n++) extra |= fx_is_windowed_cost(p->cost_id[n]);
    return extra;
}
inline int64_t fx_candidates_global(const FxProblem *p) { return p->sampling_matrix ? p->n_rows : (int64_t)p->nT * p->nV * p->nD; }
inline int64_t fx_candidates_of(const FxProblem *p) { return p->shard_count > 0 ? p->shard_count : fx_candidates_global(p); }
inline bool fx_has_boundary(const FxProblem *p) { return (p->mode & FX_MODE_ROAD_BOUNDARY) && p->n_bound > 0; }
// wave split needs whole waves per part (CPB % 64 == 0) and G in {2, 4}
inline bool fx_wave_split_possible(int G, int blk) { return (G == 2 || G == 4) && (blk / G) % 64 == 0; }
// lane-split kernels with the obstacle stage inside: the bytes of an agent's record table + its two step masks that ride in LDS
// (FX_MODE_INT_REC_LDS; fx_eval_grid_kernel.h, LSTAGE), 0 where they do not
inline size_t fx_rec_lds_bytes(bool lane_split_with_stage, int S, int K) {
    const size_t rec_bytes = sizeof(double) * (size_t)S_rec_doubles(S, std::max(K, 0));
    return (lane_split_with_stage && K > 0 && K <= 64 && rec_bytes <= FX_REC_LDS_MAX) ? rec_bytes + 16 * (size_t)S : 0;
}
// what the generic kernel stages of an agent (M knots, S samples) in LDS: the whole knot records (64 B each), the knots' arc
// lengths, the time table -- what must fit ...
inline size_t fx_generic_base_lds(int M, int S) { return sizeof(double) * ((size_t)M * (FX_REF_FIELDS + 1) + 2 + FX_TP * (size_t)S); }
inline size_t fx_generic_base_lds(const FxProblem *p) { return fx_generic_base_lds(p->M, p->N + 1); }
// ... and what a launch of it (or of its list form) asks for: an even count of arc lengths, FxStepPlan.gen_rec_lds behind them
inline size_t fx_generic_lds(int M, int S, size_t rec_lds) {
    return sizeof(double) * ((size_t)M * FX_REF_FIELDS + FX_TP * (size_t)S + (((size_t)M + 1) & ~(size_t)1)) + rec_lds;
}

// dynamic LDS of a grid-kernel workgroup of blk lanes
inline size_t fx_grid_lds(int n_agents, const FxProblem *probs, int G, int blk, int wsplit_force, bool obst_in_walk, size_t hot_block) {
    // lane split with the obstacle stage in the kernel: the record table + the two step masks behind the arc lengths
    const bool lane_split = G > 1 && !(fx_wave_split_possible(G, blk) && wsplit_force != 1);
    size_t need = 0;
    for (int a = 0; a < n_agents; a++) {
        const FxProblem *p = &probs[a];
        const size_t n_pairs = (size_t)(blk / G + p->nD - 2) / p->nD + 1;
        const size_t S = (size_t)p->N + 1;
        // time table + rows + wave-split exchange block (5 f64 + 5 u32 per slot) + tail: the knots' arc lengths
        // during the prologue, one staging block of the step's hot obstacle table per wave during the walk
        // (fx_eval_grid_kernel.h: the two share the bytes)
        need = std::max(need, sizeof(double) * FX_TP * S + 128 * n_pairs * S + (G > 1 ? (size_t)64 * blk : 0) +
                                  std::max(sizeof(double) * (((size_t)p->M + 1) & ~(size_t)1), (size_t)(blk / 64) * hot_block) +
                                  fx_rec_lds_bytes(lane_split && obst_in_walk, (int)S, p->K));
    }
    return need;
}

inline int fx_plan_upload(int n_agents, const FxProblem *probs, const FxForce &f, const FxCaps &caps, FxStepPlan *pl, char *err,
                          size_t err_len) {
    FxAgentPlan *rows = pl->agents;
    *pl = FxStepPlan();
    pl->agents = rows;
    pl->n_agents = n_agents;
    // ---- what the step holds ----
    int64_t waves1 = 0;
    bool obst_any = false, any_k = false, split_ok = true, bundle_any = false, grid_ok = true;
    const int CH = f.obst_CH ? f.obst_CH : 3;
    size_t hot_block = 0;
    for (int a = 0; a < n_agents; a++) {
        const FxProblem *p = &probs[a];
        waves1 += (fx_candidates_of(p) + 63) / 64;
        pl->any_extra |= fx_has_windowed_cost(p);
        obst_any |= p->K > 0 || fx_has_boundary(p);
        bundle_any |= (p->mode & FX_MODE_WRITE_BUNDLE) != 0;
        if (fx_has_boundary(p)) split_ok = false;
        if (p->K > 0) {
            any_k = true;
            if (p->K > 64 || !(p->mode & FX_MODE_WRITE_BUNDLE)) split_ok = false;
            pl->obs_lds = std::max(pl->obs_lds, sizeof(double) * 6 * (size_t)CH * (size_t)p->K);
        }
        if (p->sampling_matrix || p->nD < 1 || p->K > 64) grid_ok = false;   // > 64 obstacles: multi-word masks, generic kernel
        hot_block = std::max(hot_block, align_up(sizeof(double) * FX_HOT_STRIDE * (size_t)std::max(p->K, 0), 16));
    }
    // lanes per candidate: split the horizon over G lanes while the step has too few candidates to give every
    // SIMD of the chip (256 CUs x 4) a few waves; windowed (Simpson) costs need the whole horizon in one lane
    // measured on MI355X (tools/quick.py): one lane per candidate once the grid gives >= 3 waves per SIMD,
    // two lanes per candidate below that, four for tiny grids (a single wave's 31-step chain is pure latency)
    int G = 1;
    if (waves1 < 3072) G = 2;
    if (waves1 < 200) G = 4;
    // planner-sized grids are one dependent chain per lane on a mostly idle chip: spread the horizon until every lane walks
    // one or two steps (plus its carry-in step) -- tools/sweep_small.py, 5 obstacles, kernel time at 4 / 8 / 16 / 32 lanes:
    // 630 candidates 45 / 31 / 21 / 19 us; 1 260 x 51 samples 69 / 47 / 33 / 27; 3 060: 44 / 31 / 25 / 28; 4 200: 46 / 34 / 27 / 45
    if (waves1 < 100) G = 16;
    if (waves1 < 32) G = 32;
    if (f.G) G = f.G;
    if (pl->any_extra) G = 1;
    pl->G = G;
    // Obstacle stage as its own (candidate x step)-parallel kernel behind the walk (fx_obstacle_kernel.h): for grids whose
    // walk leaves most of the chip's issue slots idle (two lanes per candidate: 200 ... 3 072 waves) the K x S visits of a
    // candidate run at the walk's one or two waves per SIMD when fused; on their own they fill every SIMD.  Needs the
    // materialised planes (x, y, theta are read back), at most 64 obstacles and no road-boundary stage (that one stays in
    // the walk).  tools/c3_split.py: config 3 94.7 vs 98.6 - 105 us per step, config 5's agent with a bundle 240 vs 280 us,
    // 10 000 candidates equal, 3 060 and 1 M candidates slower.
    split_ok = split_ok && !pl->any_extra;
    if (f.obst_stage == 2 && any_k && !split_ok)
        return fx_policy_err(err, err_len, FX_ERR_INVALID_ARGUMENT, "obstacle kernel forced but not applicable (needs FX_MODE_WRITE_BUNDLE, K <= 64, no road "
                             "boundary, no windowed cost term)");
    // (a forced work decomposition -- fx_set_tuning -- runs as asked: the automatic choice only follows the automatic G)
    pl->split = any_k && split_ok && (f.obst_stage == 2 || (f.obst_stage == 0 && G == 2 && !f.G));
    pl->split_CH = CH;
    if (pl->split) { obst_any = false; hot_block = 0; }   // the walk is tuned and built without the stage (and its staging blocks)
    // large grids: 4 waves per SIMD (128 VGPRs, a few spills) beats 2 at full VGPR budget; small grids are
    // latency-bound with 1-2 waves per SIMD anyway and run faster unspilled
    // with the obstacle stage the walk needs ~220 VGPRs: three waves per SIMD (168 VGPRs, few spills) is the best
    // trade at scale, four spill inside the obstacle loop (tools/obst_sweep.py)
    // a materialised bundle makes the walk store-bound: more resident waves only add spills (1 M candidates, Mode B:
    // 651 us at 2 waves per SIMD, 697 us at 4 -- tools/sweep_1m_modeB.py)
    // ... but with the obstacle stage in the walk as well (the north star as written) the kernel is bound by the vector unit and
    // by latency as much as by its stores: the third wave per SIMD pays (168 registers, no vector spill): 1 062 -> 1 004 us
    // same-box, tools/ns_wpe.py
    pl->wpe = f.wpe ? f.wpe : (waves1 >= 3072 ? (obst_any ? 3 : (bundle_any ? 2 : 4)) : 2);
    // grid kernel: sampling ranges, no windowed costs, and the longitudinal rows of a workgroup fit in LDS.
    // Workgroup size: the smallest of 64/128/256 lanes whose LDS footprint still lets a CU hold the target
    // number of waves (small workgroups balance small grids at wave granularity).
    grid_ok = grid_ok && !pl->any_extra;
    size_t lds_need = 0;
    int block = FX_BLOCK;
    if (grid_ok) {
        auto lds_for = [&](int blk) { return fx_grid_lds(n_agents, probs, G, blk, f.wsplit, obst_any, hot_block); };
        const int want_waves = 4 * pl->wpe;
        const size_t lds_static = 256;  // static LDS of the kernels (reductions)
        const size_t lds_cap = (160 * 1024) / 2 - 2 * lds_static;  // two workgroups per CU
        block = 0;
        int best_waves = 0;
        const int order_big[3] = {256, 128, 64}, order_small[3] = {128, 256, 64};
        for (int bi = 0; bi < 3; bi++) {
            // two parts on two waves (G = 2, wave split) with the obstacle stage: 128-lane workgroups -- one wave per part --
            // finish 3 - 8 % earlier than 256-lane ones (config 3: 88 - 95 vs 96 us); without obstacles they are slower
            // (config 2: 48.6 vs 42.1 us, select-only 38.4 vs 29.1) -- tools/sweep_tuning.py, tools/c3.py
            const int blk = (G >= 8 || (G == 2 && obst_any) ? order_small : order_big)[bi];
            if (f.wsplit == 2 && (G == 2 || G == 4) && !fx_wave_split_possible(G, blk)) continue;   // a forced wave split needs whole waves per part
            const size_t need = lds_for(blk);
            const int by_lds = (int)((160 * 1024) / (need + lds_static));
            const int waves = by_lds * (blk / 64);
            if (waves >= want_waves && need <= lds_cap) { block = blk; lds_need = need; break; }
            // nothing reaches the target (few lateral samples per pair -> many rows): keep the workgroup size that
            // holds the most waves per CU among those whose rows fit at all
            if (need <= lds_cap && waves > best_waves) { best_waves = waves; block = blk; lds_need = need; }
        }
        if (f.block) { block = f.block; lds_need = lds_for(block); }
        if (!block) { block = FX_BLOCK; lds_need = lds_for(block); }
        if (lds_need > lds_cap) grid_ok = false;   // at least two workgroups per CU
    }
    if (f.variant == 1) grid_ok = false;
    if (f.variant == 2 && !grid_ok)
        return fx_policy_err(err, err_len, FX_ERR_INVALID_ARGUMENT, "grid kernel forced but not applicable (G=%d block=%d rows+tables need %zu B of LDS per workgroup)", G, block, lds_need);
    pl->use_grid = grid_ok;
    pl->lds = std::max(lds_need, f.lds_pad);
    pl->block = grid_ok ? block : FX_BLOCK;
    const bool ws_possible = grid_ok && fx_wave_split_possible(G, pl->block);
    pl->wsplit = ws_possible && f.wsplit != 1;
    if (f.wsplit == 2 && !ws_possible && G > 1) return fx_policy_err(err, err_len, FX_ERR_INVALID_ARGUMENT, "wave split forced but not applicable");
    // lane-split kernels with the obstacle stage inside: which agents' record tables ride in LDS.  Grid kernel: fx_grid_lds has made
    // room; generic kernel (>= 4 lanes per candidate): behind the knots and the time table where everything still fits a CU
    bool rec_rule = pl->use_grid && G > 1 && !pl->wsplit;
    if (!pl->use_grid && G >= 4) {
        size_t base_max = 0, need = 0;
        for (int a = 0; a < n_agents; a++) {
            base_max = std::max(base_max, fx_generic_base_lds(&probs[a]));
            need = std::max(need, fx_rec_lds_bytes(true, probs[a].N + 1, probs[a].K));
        }
        if (need && base_max + need <= (size_t)160 * 1024 - 2048) { rec_rule = true; pl->gen_rec_lds = need; }
    }
    // ---- the agents' places ----
    const int CPB = pl->block / G;
    int64_t cand_off = 0, block_off = 0;
    bool all_deferred = n_agents > 0;
    pl->fusable = true;
    for (int a = 0; a < n_agents; a++) {
        const FxProblem *p = &probs[a];
        FxAgentPlan &r = pl->agents[a];
        r = FxAgentPlan();
        const int S = p->N + 1;
        const int64_t C_global = fx_candidates_global(p);
        if (p->shard_count < 0 || p->shard_begin < 0 || (p->shard_count > 0 && p->shard_begin + p->shard_count > C_global))
            return fx_policy_err(err, err_len, FX_ERR_INVALID_ARGUMENT, "shard [%lld, +%lld) outside the grid of %lld candidates",
                                 (long long)p->shard_begin, (long long)p->shard_count, (long long)C_global);
        const int64_t C = r.C = fx_candidates_of(p);
        r.g_base = p->shard_count > 0 ? p->shard_begin : 0;
        if (p->N > caps.max_steps) return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "N=%d exceeds context capacity %d", p->N, caps.max_steps);
        if (p->M > caps.max_knots) return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "M=%d reference knots exceed capacity %d", p->M, caps.max_knots);
        if (p->K > caps.max_obs || (p->K > 0 && p->P > caps.max_pred))
            return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "obstacles K=%d P=%d exceed capacity %d x %d", p->K, p->P, caps.max_obs, caps.max_pred);
        // only the generic kernel stages the whole knot records (64 B each) in LDS; the grid kernel keeps 8 B per knot and its
        // LDS need was checked when it was chosen above
        if (!pl->use_grid && fx_generic_base_lds(p) > 160 * 1024 - 1024)
            return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "reference with %d knots does not fit the 160 KiB LDS of the generic kernel (sampling matrix / "
                                 "windowed costs); resample the reference or use sampling ranges", p->M);
        r.ld = (int64_t)align_up((size_t)std::max<int64_t>(C, 1), 64);
        if (cand_off + r.ld > caps.total_ld)
            return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "candidates exceed context capacity %lld", (long long)caps.max_cand);
        r.cand_off = cand_off; r.block_off = block_off;
        r.mode = p->mode;
        if (p->K <= 0 || !p->obs_hull || !p->obs_nhull) r.mode &= ~FX_MODE_COLLISION;
        if (!fx_has_boundary(p)) r.mode &= ~FX_MODE_ROAD_BOUNDARY;
        r.n_blocks = r.walk_blocks = (int)((C + CPB - 1) / CPB);
        r.deferred = pl->split && p->K > 0;
        if (fx_rec_lds_bytes(rec_rule && !r.deferred, S, p->K)) r.mode |= FX_MODE_INT_REC_LDS;
        all_deferred = all_deferred && r.deferred;
        if (r.deferred) {   // the obstacle kernel writes this agent's arg-min partials: one per tile of 64 candidates
            r.mode |= FX_MODE_INT_DEFER_OBST;
            if (f.obst_chunk_index) r.mode |= FX_MODE_INT_CHUNK_INDEX;
            const int n_tiles = (int)((C + 63) / 64), NC = (S - 1 + CH - 1) / CH;
            const int NC_alloc = std::max(NC, (S - 1 + 2) / 3);   // (the one-launch step picks its own steps per item: 3, 5 or 8)
            r.n_blocks = n_tiles;
            pl->obs_blocks = std::max(pl->obs_blocks, n_tiles * NC);
            pl->obs_tiles = std::max(pl->obs_tiles, n_tiles);
            pl->obs_wg_waves = std::max(pl->obs_wg_waves, NC);
            r.obs_part_off = pl->obs_part_n; r.obs_colm_off = pl->obs_colm_n; r.obs_tick_off = pl->obs_tick_n;
            pl->obs_part_n += (size_t)NC_alloc * (size_t)r.ld;
            pl->obs_colm_n += (size_t)NC_alloc * (size_t)n_tiles;
            pl->obs_tick_n += (size_t)n_tiles;
        }
        if (block_off + r.n_blocks > caps.max_blocks_total)
            return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "agent %d: %lld workgroups exceed the partial-result capacity %lld", a,
                                 (long long)(block_off + r.n_blocks), (long long)caps.max_blocks_total);
        if (r.mode & FX_MODE_WRITE_BUNDLE) {
            if ((uint64_t)r.ld * 8u >= (1ull << 32))  // the walk addresses a row with a 32-bit byte offset per lane
                return fx_policy_err(err, err_len, FX_ERR_CAPACITY, "agent %d: %lld candidates with a materialised bundle (rows are limited to 4 GiB)", a, (long long)C);
            r.planes_off = pl->planes_bytes;
            pl->planes_bytes += sizeof(double) * FX_NUM_PLANES * (size_t)S * (size_t)r.ld;
            pl->any_bundle = true;
        }
        pl->any_obst |= (p->K > 0 && !r.deferred) || (r.mode & FX_MODE_ROAD_BOUNDARY);
        if (r.n_blocks == 0 || r.deferred) pl->fusable = false;
        // candidates per agent up to which the agent's last workgroup counts the collisions in front of the winner itself (it re-reads
        // the agent's flag words); larger steps keep fx_select_kernel's slices.  Measured (tools/probe_timeline.py, closed_loop_timing.py):
        // the tail costs ~6.5 us at 630 candidates and 8 - 10 us at 11 000, the selection kernel + gather behind a launch gap ~8.5 - 10 us
        // whatever the size -- plan() 70 -> 63 us at 630 candidates, 81 -> 84 us at 11 220: the bound sits between them
        if (r.mode & FX_MODE_COLLISION) {
            pl->count = true;
            if (C > f.tail_max_c && !f.fuse_any_size) pl->fusable = false;
        }
        pl->max_blocks = std::max(pl->max_blocks, r.walk_blocks);
        pl->M_max = std::max(pl->M_max, p->M);
        pl->K_max = std::max(pl->K_max, std::max(p->K, 0));
        pl->S_max = std::max(pl->S_max, S);
        pl->C_max = std::max(pl->C_max, C);
        cand_off += r.ld;
        block_off += r.n_blocks;
    }
    // plane stores: write-through while the step's whole bundle is small (FX_STORE_WT_MAX_BYTES, measured), else write-back
    pl->wt = pl->planes_bytes && (f.store == 2 || (f.store == 0 && pl->planes_bytes <= FX_STORE_WT_MAX_BYTES));
    for (int a = 0; a < n_agents && pl->wt; a++) pl->agents[a].mode |= FX_MODE_INT_STORE_WT;
    // the whole step in one launch (fx_step_kernel.h): the split step of the tuned two-lanes-per-candidate walk with a write-through
    // bundle, every agent's obstacle stage deferred; whether the device holds the launch is asked when it is sized (fx_evaluate)
    // (opt-in: measured slower than the three launches on config 3, fx_step_kernel.h -- `force` 2 or FX_STEP_KERNEL=1)
    // (a split step whose agents are all deferred has a bundle, at most 64 obstacles, no windowed cost and no stage left in the walk;
    // the wave split runs in the grid kernel only)
    pl->step_kernel_ok = f.step_kernel == 2 && pl->split && all_deferred && G == 2 && pl->wsplit && pl->block == FX_BLOCK && pl->wpe == 2 &&
                         pl->wt && pl->obs_blocks > 0;
    return FX_OK;
}

// The part decided per evaluation (fx_plan_and_package switches the package on for one call).
inline FxLaunchPlan fx_plan_launches(const FxStepPlan &pl, const FxForce &f, bool package_enabled) {
    FxLaunchPlan L;
    L.eval_launched = pl.max_blocks > 0;
    // one launch when no agent needs the collision-ordered count of the selection kernel: the evaluation kernel's
    // last workgroup reduces and publishes (fx_eval_kernel.h, "fused selection")
    L.fused = f.fuse_enabled && pl.fusable && L.eval_launched;
    L.pkg = package_enabled && pl.any_bundle;
    // the agent's last workgroup ends the step (fx_tail.h): collision count where a collision stage ran in this kernel, winner
    // package where the bundle is stored write-through -- a planner-sized step with everything on is ONE launch
    // (the tail is compiled into the planner-sized decompositions only, FX_TAIL_IN_KERNEL: a step of another decomposition that
    // needs the collision count keeps the selection kernel, one that only needs the package keeps the package kernel)
    const bool tail_kernel = FX_TAIL_IN_KERNEL(pl.G, pl.any_extra);
    if (L.fused && pl.count && !tail_kernel) L.fused = false;
    if (L.fused && tail_kernel) {
        if (pl.count) L.tail |= FX_TAIL_COUNT;
        if (L.pkg && pl.wt) L.tail |= FX_TAIL_PACKAGE;
    }
    const bool pkg_in_tail = (L.tail & FX_TAIL_PACKAGE) != 0;
    L.try_step_kernel = pl.step_kernel_ok;   // (its deferred agents rule the fused selection out)
    L.obstacle = pl.split && pl.obs_blocks > 0;
    if (L.obstacle) {
        // one workgroup per tile (the chunks meet in LDS) where the horizon's chunks fit a workgroup; else single-wave items
        // (measured, tools/c3_split.py: config 3 34.2 -> 32.5 us, config 4's batch 15.6 -> 13.2 us; a config-5 agent with a bundle
        // -- 1 617 tiles -- 102 -> 159 us and the 1 M grid 374 -> 524 us: ten-wave workgroups schedule badly once there are more
        // tiles than the chip holds at once, so the automatic choice takes them up to 1 024 tiles per launch)
        const int wg_mode = f.obst_wg ? f.obst_wg : ((int64_t)pl.obs_tiles * pl.n_agents <= 1024 ? 2 : 1);
        const size_t lds_wg = align_up((size_t)pl.obs_wg_waves * (pl.obs_lds + 64 * sizeof(double) + sizeof(unsigned long long)), 16);
        // the workgroup's waves each keep their slice of the staging area: five steps per item with 64 obstacles and eleven or more
        // chunks would ask for more than a CU's 160 KB (minus the kernel's static LDS) -- such a step runs as single-wave items
        const bool wg = wg_mode == 2 && pl.obs_wg_waves <= 16 && lds_wg <= (size_t)160 * 1024 - 1024;
        L.obs_wg = wg ? pl.obs_wg_waves : 0;
        L.obs_lds = wg ? lds_wg : pl.obs_lds;
    }
    // with a package the selection's publishing workgroup gathers the winner's arrays itself (no further launch)
    L.select = !L.fused;
    // fused selection without the tail's write-through hand-off (forced write-back plane stores) publishes while other waves'
    // plane stores may still be in flight: the gather runs as its own small kernel behind the evaluation; fx_finish waits for
    // its sequence word
    L.package = L.fused && L.pkg && !pkg_in_tail;
    L.one_launch = L.fused && (!L.pkg || pkg_in_tail);
    return L;
}

static const int FX_STEP_KERNEL_CHS[3] = {3, 5, 8};   // steps per obstacle item the one-launch step is built for
// dynamic LDS of the one-launch step at CH steps per item: the walk's, or its waves' staging areas (FX_STEP_ITEM_DOUBLES)
inline size_t fx_step_kernel_lds(const FxStepPlan &pl, int CH) {
    return std::max(pl.lds, (size_t)(FX_BLOCK / 64) * sizeof(double) * 6 * (size_t)CH * (size_t)pl.K_max);
}
// The one-launch step's sizing: (tile, chunk of CH steps) items over all waves of the launch, in as few rounds as the resident
// workgroups allow -- the list's length is the previous step's (a planner's consecutive steps differ little; last_live < 0: none
// yet), two thirds of the grid at first.  cap[q]: workgroups of the kernel the device holds at once at FX_STEP_KERNEL_CHS[q] steps
// per item and fx_step_kernel_lds bytes.
inline FxStepKernelSize fx_plan_step_kernel(const FxStepPlan &pl, const FxForce &f, int64_t last_live, const int cap[3]) {
    const int64_t live_est = last_live >= 0 ? std::min(last_live, pl.C_max) : (2 * pl.C_max + 2) / 3;
    const int tiles_est = (int)std::max<int64_t>(1, (live_est + 63) / 64);
    FxStepKernelSize best;
    int best_score = 1 << 30;
    for (int q = 0; q < 3; q++) {
        const int CH = FX_STEP_KERNEL_CHS[q];
        if (f.step_kernel_CH && f.step_kernel_CH != CH) continue;
        const int cap_agent = cap[q] / std::max(pl.n_agents, 1);
        if (cap_agent < pl.max_blocks) continue;   // the walk alone does not fit at once: three launches
        const int NC = (pl.S_max - 1 + CH - 1) / CH;
        const int64_t items = (int64_t)tiles_est * NC;   // (one tile x one chunk per wave)
        const int blocks = (int)std::min<int64_t>(cap_agent, std::max<int64_t>(pl.max_blocks, (items + FX_BLOCK / 64 - 1) / (FX_BLOCK / 64)));
        const int rounds = (int)((items + (int64_t)blocks * (FX_BLOCK / 64) - 1) / ((int64_t)blocks * (FX_BLOCK / 64)));
        const int score = rounds * CH;
        if (score < best_score) { best_score = score; best.CH = CH; best.blocks = blocks; best.lds = fx_step_kernel_lds(pl, CH); }
    }
    return best;
}
// the one-launch step takes the evaluation's place: nothing follows it
inline void fx_take_step_kernel(FxLaunchPlan &L, const FxStepKernelSize &sz) {
    L.step_kernel = L.one_launch = true;
    L.step_blocks = sz.blocks; L.step_CH = sz.CH; L.step_lds = sz.lds;
    L.obstacle = L.select = L.package = false;
    L.obs_wg = 0; L.obs_lds = 0;
}

// fx_step_info_ex's 16 numbers (include/fxplan.h); stage_path: how the latest inputs reached the device
inline void fx_step_info_of(const FxStepPlan &pl, const FxLaunchPlan &L, int stage_path, int64_t *out16) {
    const int64_t v[16] = {pl.use_grid, pl.G, pl.wpe, pl.block, pl.wsplit, L.fused, pl.max_blocks, pl.n_agents, L.pkg, (int64_t)pl.lds,
                           pl.split, pl.split_CH, pl.obs_blocks, (int64_t)pl.obs_lds, L.obs_wg, L.tail | ((int64_t)stage_path << 8)};
    std::copy(v, v + 16, out16);
    if (L.step_kernel) {   // the whole step in one launch: steps per item, waves, LDS of THAT kernel; bit 16 says so
        out16[11] = L.step_CH; out16[12] = (int64_t)L.step_blocks * (FX_BLOCK / 64); out16[13] = (int64_t)L.step_lds; out16[14] = 0;
        out16[15] |= 1 << 16;
    }
}
