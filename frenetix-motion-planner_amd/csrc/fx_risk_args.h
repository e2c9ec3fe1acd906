// fx_risk_args.h -- what the host code of the trajectory risk (fx_api_risk.hip), its launcher (fx_kernels.hip) and its kernels
// (fx_risk_kernel.h) share: the layout of the records the host builds and the kernels read, the arguments of the candidate walk
// and the argument blocks of the risk-cost kernel, the responsibility re-sum and the prediction-probability pass, and the row
// tables of the four passes that take several agents in one call.  DESIGN.md sections 11, 13, 16, 17, 18, 19, 20 and 21.
#pragma once

#include <stdint.h>

#include "../../include/fxplan.h"

// record of one (obstacle, ego step i): doubles
#define FXR_M0X 0    // means: pos[i-1], pos[i-1] +- (cos, sin)(yaw[i]) length / 2
#define FXR_SX 6
#define FXR_SY 7
#define FXR_RHO 8
#define FXR_BRANCH 9  // 0: rho == 0, 1: |rho| < 0.925, 2: 0.925 <= |rho| < 1, 3: |rho| == 1
#define FXR_NG 10     // Gauss-Legendre half nodes (3, 6, 10)
#define FXR_VALID 11  // i < len(pos_list)
#define FXR_IV 12     // inverse covariance (Mahalanobis mode)
#define FXR_ASR 16    // branch 1: asin(rho) / 2; branch 2: 1 - rho^2
#define FXR_A 17      // branch 2: sqrt(1 - rho^2)
#define FXR_N1 18     // branch 1: sin(asr (1 - x_j)), then sin(asr (1 + x_j)); branch 2: xs_j = (a/2 (1 -+ x_j))^2
#define FXR_N2 38     // branch 2: sqrt(1 - xs_j)
#define FXR_STRIDE 58

// per obstacle: doubles
#define FXO_LEN 0
#define FXO_WID 1
#define FXO_MASS 2
#define FXO_CLS 3
#define FXO_NPOS 4
#define FXO_STRIDE 8

// what the candidate walk (fx_risk_item_kernel / fx_risk_items_finish_kernel) reads, device pointers
struct RiskWalkArgs {
    const double *planes;      // [FX_NUM_PLANES][S][ld] of the agent
    int64_t ld;
    int32_t S;
    int64_t n;
    const int64_t *ids;        // [n] or null: every candidate, NaN rows for the unselected ones
    const uint32_t *flags;     // [ld] of the agent
    const double *rec;         // [K][S][FXR_STRIDE]
    const double *obs;         // [K][FXO_STRIDE]
    const double *pos;         // [K][P][2]
    const double *yaw, *vo;    // [K][P]
    int32_t K, P;
};

// the items of the candidate walk, device pointers
struct RiskItemArgs {
    const FxRiskParams *params;// the call's parameters, in device memory
    double *part;              // [K][chunks][NV][nb] partials of one batch of nb candidates (NV = 2, detail 7)
    int64_t nb;                // candidates per batch: whole tiles of 64
    int32_t cs, chunks;        // steps per chunk, chunks = ceil(max(S - 1, 1) / cs)
    uint32_t need;             // ids == null: the flags a candidate needs; the others get NaN rows
};

// arguments of the responsibility term's re-sum (fx_resp_finish_kernel), device pointers
struct RespSumArgs {
    int64_t n;
    const int64_t *ids;        // [n] or null: every candidate, NaN rows for the ones that lack a flag of `need`
    const uint32_t *flags;     // [ld]
    uint32_t need;
    const double *resp;        // [n] responsibility cost (row 4 of the cost pass's output)
    const double *pred;        // [n] prediction entry to use instead of the step's own, or null
    const double *costmap;     // [n_cost][ld] raw cost rows of the step
    int64_t ld;
    int32_t n_cost, n_pred;    // n_pred: position of FX_COST_PREDICTION in the cost list, -1 without one
    int32_t at;                // the term is added in front of entry `at` of the cost list (n_cost: behind all)
    int32_t deferred;          // the step closed its sum in the obstacle kernel (FX_MODE_INT_DEFER_OBST)
    double cost_w[FX_NUM_COSTS], w_resp;
    double *resp_out, *total;  // [n]
};

struct RiskCostArgs {
    const double *col;         // [4][K][n]: ego_risk_max | obst_risk_max | ego_harm_max | obst_harm_max of the detail pass
    int64_t n;
    const int64_t *ids;        // [n] or null: every candidate, NaN rows for the unselected ones
    const uint32_t *flags;     // [ld] of the agent
    const double *planes;      // [FX_NUM_PLANES][S][ld] of the agent
    int64_t ld;
    int32_t S, K;
    const double *bh_in;       // [n] boundary harm of the caller, or null
    const int32_t *bstep;      // [ld] first step outside the road: boundary harm derived from it (null: 0 without bh_in)
    double bh_c, bh_s;
    int32_t resp_mode;         // FX_RISK_RESP_*
    int32_t n_entries;         // reach-set obstacles
    const double *resp;        // [K] 0 / 1 (action-space mode)
    const int32_t *entry_obs;  // [n_entries] obstacle index of the entry
    const int32_t *entry_off;  // [n_entries + 1] its parts
    const int32_t *part_step;  // [n_parts] ego step index of the part
    const int32_t *vert_off;   // [n_parts + 1]
    const double *verts;       // [n_verts][2]
    double w[5], eps, scale;
    double *out;               // [7][n]: bayes | equality | maximin | ego | responsibility | total | boundary_harm
};

// arguments of the prediction-probability pass (fx_predprob_kernel.h), device pointers
struct PredProbArgs {
    const double *planes;      // [FX_NUM_PLANES][S][ld] of the agent (or of its sparse set)
    int64_t ld;
    int32_t S, K;
    int64_t n;                 // listed candidates (or C)
    const int64_t *ids;        // [n] or null: every candidate, NaN rows for the ones without FX_FLAG_COSTED
    const uint32_t *flags;     // [ld]
    const double *rec;         // [K][S][FXR_STRIDE], MVN mode
    double ego_length, ego_width;
    int32_t source;            // FX_PRED_SOURCE_*
    // the re-sum
    const double *costmap;     // [n_cost][ld] raw cost rows of the step
    int32_t n_cost, n_pred;    // n_pred: position of FX_COST_PREDICTION in the cost list
    int32_t deferred;          // the step closed its sum in the obstacle kernel (FX_MODE_INT_DEFER_OBST)
    double cost_w[FX_NUM_COSTS];
    // scratch and outputs
    double *step;              // [K][S - 1][nb] probabilities of one batch of nb candidates
    int64_t nb;
    double *prob, *prob_obs, *total;   // [n], [K][n], [n]
};

// The pass over several agents in one call (fx_eval_prediction_prob_batch): one row per (round, agent with
// candidates in it) in device memory, the rows of a round consecutive and in call order (fx_item_rounds, fx_pass.h).
struct PredProbRow {
    PredProbArgs a;            // of the agent: ids and prob_obs null, n = C, prob / total the agent's rows of the call's outputs,
                               // step the agent's segment of the round's scratch, nb = count rounded up to whole tiles
    int64_t first, count;      // the agent's candidates of this round
    int32_t cs, chunks;        // steps per chunk, chunks = ceil(max(S - 1, 1) / cs); chunks = 0: the row has no item
    int64_t item0;             // first item of the row in the round's flat index; its items: (nb / 64) x chunks x K, tile fastest
    int32_t fin0;              // first workgroup of the row in the round's finish launch; it has ceil(count / 256)
};
// Where the tables of a batched call lie, device pointers (host only: the launchers read it): what the four passes over several
// agents share.  The rounds are FxItemRound (fx_pass.h).
template <class Row>
struct BatchTable {
    const Row *rows;           // [n_rows], all rounds
    const int64_t *item0;      // [n_rows] the rows' item0, compact: a wave looks its row up with one load
    const int32_t *fin0;       // [n_rows] the rows' fin0
    const int32_t *agent_row;  // [n_agents] a row of the agent (any of them: an arg-min reads what is the agent's in it), -1 without one
    int32_t n_agents;
};
typedef BatchTable<PredProbRow> PredProbBatchArgs;

// The responsibility pass over several agents in one call (fx_eval_responsibility_cost_batch): the table of
// the prediction-probability batch with the walk's arguments in the rows.  One row per (round, agent with candidates in it), the
// rows of a round consecutive and in call order (fx_item_rounds, fx_pass.h).
struct RiskBatchRow {
    RiskWalkArgs w;            // of the agent: ids null, n = C
    RiskItemArgs it;           // of the agent: need = FX_FLAG_COSTED, params its FxRiskParams in the block, part its segment of the
                               // round's scratch [K][chunks][7][nb], nb = count rounded up to whole tiles, cs / chunks of its OWN size
    int64_t first, count;      // the agent's candidates of this round
    int64_t item0;             // first item of the row in the round's flat index; its items: (nb / 64) x chunks x K, tile fastest
    int32_t fin0;              // first workgroup of the row in the round's finish launch; it has ceil(count / 256)
    int32_t items;             // 0: the row runs no item (K = 0 or S = 1)
    double *ego, *obst, *occ;  // [C] of the agent: what the finish kernel writes
    double *col;               // [4][K][C] of the agent
};
// the table and what the launches behind the rounds cover (the arg-min reads `sum`, not agent_row)
struct RiskBatchArgs {
    BatchTable<RiskBatchRow> t;
    const RiskCostArgs *cost;  // [n_agents] of the cost kernel, ids null: every row is evaluated
    const RespSumArgs *sum;    // [n_agents] of the re-sum and the arg-min
    const int32_t *blk0;       // [n_agents] first workgroup of 256 of the agent in the cost and re-sum launches; it has ceil(C / 256)
    int32_t blocks;            // of all agents
};

// The plain risk pass over several agents in one call, each with an id list or none (fx_eval_risk_batch):
// the rows are RiskBatchRow as above -- its layout is the existing batch kernels' -- with, per agent, w.ids its list in the block
// (positions in its sparse set where the step stored no bundle) or null, w.n the list's length or C, first / count list positions,
// it.need = VALID | FEASIBLE | RETURNED, it.part [K][chunks][2][nb], ego / obst the agent's rows of the call's concatenated
// outputs, occ and col null.  Its arg-min reads ego, obst, w.n and w.ids of the agent's row.
typedef BatchTable<RiskBatchRow> RiskListBatchArgs;

// The detail and cost passes over several agents in one call, each with an id list or none and with cost parameters or none
// (fx_eval_risk_costs_batch): the rows are RiskBatchRow with the lists of section 20 in w.ids and the
// detail pass's parts -- it.part [K][chunks][7][nb], occ the agent's rows of the call's concatenated outputs, col the agent's
// [4][K][n].  The cost pass runs over the agents that have cost parameters alone.
// The caller's columns are concatenated per column -- agent i's [K_i][n_i] at the sum of K_b n_b of the agents before it -- while
// items_finish_body and cost_body index an agent's four columns as ONE block [4][K][n]: a segment is one plane of one agent.
struct RiskCopySeg {
    const double *src;         // [n] plane q of the agent's block
    double *dst;               // its place in column q of the call
    int64_t n;                 // K n of the agent
};
struct RiskCostBatchArgs {
    BatchTable<RiskBatchRow> t;
    const RiskCostArgs *cost;  // [n_cost] of the agents with cost parameters, in call order; ids the agent's list or null
    const int32_t *blk0;       // [n_cost] first workgroup of 256 of the agent in the cost launch; it has ceil(n / 256)
    int32_t n_cost, blocks;    // blocks: of all agents with cost parameters
    const RiskCopySeg *seg;    // [n_seg] the agents' column planes on their way into the call's concatenated columns, or null
    const int32_t *seg_blk0;   // [n_seg] first workgroup of the segment in the gather launch; it has ceil(n / 1024)
    int32_t n_seg, seg_blocks; // seg_blocks 0: the caller asked for no column
};
