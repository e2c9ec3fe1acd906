// fx_cost_sum.h -- the weighted cost of a candidate re-summed from its raw cost rows (FX_MODE_WRITE_COSTMAP), in the order and with the
// operations of the plan step: what fx_predprob_finish_kernel (fx_predprob_kernel.h, one row replaced) and the re-score kernels
// (fx_rescore_kernel.h, other weights) share.
//
//   undeferred (finish_candidate, fx_eval_kernel.h):   sum = -0.0; sum += w[m] * raw[m] per term, in the cost list's order; 0.0 + sum
//   deferred (FX_MODE_INT_DEFER_OBST, the obstacle stage closed the sum: fx_obstacle_kernel.h): the terms behind the prediction were
//   added up by the walk from 0.0 (cost_tail) and join the sum as ONE addend, behind the prediction's own.
//
// A caller starts from FxCostSum{}, adds the list's terms in order and closes.  A: what says how the step summed -- .deferred, .n_pred
// (position of the prediction term), .n_cost -- read through the reference where the rule needs them (PredProbArgs, fx_risk_args.h;
// fxrs::Dims).  The sums travel by value, not through references, and `tail` stands first: fx_predprob_finish_kernel's instructions
// and registers are then what they were while these lines stood in its body, but for the order of two independent selects in its
// loop (the compiler simplifies a helper before it inlines it; one that adds through references comes out as ONE addition behind
// a select -- other code).  DESIGN.md section 23.
#pragma once

#include <hip/hip_runtime.h>

struct FxCostSum {
    double tail = 0.0, sum = -0.0;
};

// term m of the list: weight * raw cost
template <class A>
__device__ __forceinline__ FxCostSum fx_cost_sum_add(const A &a, FxCostSum s, const int m, const double w, const double raw) {
    const double t = w * raw;
    if (a.deferred && m > a.n_pred) s.tail += t;
    else s.sum += t;
    return s;
}
// behind the last term: the tail joins as one addend; the total (two steps, so that a caller can store between them as
// fx_predprob_finish_kernel always has; fx_cost_sum_close is both)
template <class A>
__device__ __forceinline__ FxCostSum fx_cost_sum_join(const A &a, FxCostSum s) {
    if (a.deferred && a.n_pred + 1 < a.n_cost) s.sum += s.tail;
    return s;
}
__device__ __forceinline__ double fx_cost_sum_total(const FxCostSum s) { return 0.0 + s.sum; }
template <class A>
__device__ __forceinline__ double fx_cost_sum_close(const A &a, const FxCostSum s) {
    return fx_cost_sum_total(fx_cost_sum_join(a, s));
}
