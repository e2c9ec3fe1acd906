// fx_risk_args.h -- argument block of the risk-cost kernel (fx_risk_kernel.h), shared by the host code that fills it
// (fx_api_risk.hip) and the launcher (fx_kernels.hip).  DESIGN.md section 13.
#pragma once

#include <stdint.h>

#include "../../include/fxplan.h"

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
