// fx_selftest_kernel.h -- the device arithmetic primitives, one at a time (included by fx_kernels.hip).
//
// One elementwise kernel with an op code: element i of the input arrays goes through ONE primitive of the product headers --
// fx_math.h (atan, atan_small, atan_small_tab, sincos), fx_walk.h (rcp_nr, rcp_pred, fdiv, sqrt_rsqrt), fx_eval_kernel.h
// (div_rcp, np_round5, wrap_pm_2pi, obb_hull, obb_overlap) -- and the results land in the output arrays.  Every op calls the
// function the evaluation kernels inline, never a copy, in the same translation unit and under the same compiler flags, so a
// changed constant, a lost Newton step or a toolchain that starts contracting these expressions shows here in the last bit,
// where a plan step compared at 1e-9 cannot see it (tests/test_device_math.py; DESIGN.md section 2, "The device primitives").
// Nothing on the product path launches it (fx_device_selftest, fx_api_host.hip).
#pragma once

#include "fx_eval_kernel.h"
#include "fx_walk.h"

// (FX_SELFTEST_* op codes: include/fxplan.h; SelftestArgs and the ops' array shapes: fx_device.h)
__global__ __launch_bounds__(256) void fx_selftest_kernel(int op, int n, SelftestArgs a) {
    // the LDS copy of atan's polynomial block, filled as fx_eval_grid_kernel.h fills it
    __shared__ __attribute__((aligned(16))) double sh_atan_k[FX_ATAN_K];
    const int tid = threadIdx.x;
    if (tid < FX_ATAN_K) sh_atan_k[tid] = fxm::fx_ktab[FX_ATAN_K0 + tid];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + tid;
    if (i >= n) return;
    const double x = a.in[0][i];   // (the wide ops re-read their own layout below; element i exists in every layout)
    switch (op) {
    case FX_SELFTEST_ATAN: a.out[0][i] = fxm::atan<false>(x); break;
    case FX_SELFTEST_ATAN_TAB: a.out[0][i] = fxm::atan<true>(x); break;
    case FX_SELFTEST_ATAN_SMALL: a.out[0][i] = fxm::atan_small(x); break;
    case FX_SELFTEST_ATAN_SMALL_TAB: a.out[0][i] = fxm::atan_small_tab(x, (fxm::lds_cptr)sh_atan_k); break;
    case FX_SELFTEST_SINCOS: fxm::sincos<false>(x, &a.out[0][i], &a.out[1][i]); break;
    case FX_SELFTEST_SINCOS_TAB: fxm::sincos<true>(x, &a.out[0][i], &a.out[1][i]); break;
    case FX_SELFTEST_RCP_NR: a.out[0][i] = fxk::rcp_nr(x); break;
    case FX_SELFTEST_RCP_PRED: a.out[0][i] = fxk::rcp_pred(x); break;
    case FX_SELFTEST_FDIV: a.out[0][i] = fxk::fdiv(x, a.in[1][i]); break;
    case FX_SELFTEST_SQRT_RSQRT: {
        double sq, rsq;
        fxk::sqrt_rsqrt(x, sq, rsq);
        a.out[0][i] = sq; a.out[1][i] = rsq;
        break;
    }
    case FX_SELFTEST_DIV_RCP: {   // as make_lon_row calls it: the reciprocal comes from rcp_nr
        const double b = a.in[1][i];
        a.out[0][i] = fxk::div_rcp(x, b, fxk::rcp_nr(b));
        break;
    }
    case FX_SELFTEST_NP_ROUND5: a.out[0][i] = fxk::np_round5(x); break;
    case FX_SELFTEST_WRAP_PM_2PI:
        // the function is a loop of |a| / 2 pi rounds that never ends for +-inf or 1e300: the host refuses such input
        // (fx_device_selftest) and the kernel does not enter the loop with it either
        a.out[0][i] = fabs(x) <= FX_SELFTEST_WRAP_MAX ? fxk::wrap_pm_2pi(x) : __builtin_nan("");
        break;
    case FX_SELFTEST_OBB_HULL: {
        const double *p = a.in[0] + 4 * (size_t)i, *q = a.in[1] + 4 * (size_t)i, *h = a.in[2] + 2 * (size_t)i;
        const fxk::Obb o = fxk::obb_hull(p[0], p[1], p[2], p[3], q[0], q[1], q[2], q[3], h[0], h[1]);
        a.out[0][i] = o.cx; a.out[1][i] = o.cy; a.out[2][i] = o.ex; a.out[3][i] = o.ey; a.out[4][i] = o.h1; a.out[5][i] = o.h2;
        break;
    }
    case FX_SELFTEST_OBB_OVERLAP: {
        const double *p = a.in[0] + 6 * (size_t)i;
        const fxk::Obb o = {p[0], p[1], p[2], p[3], p[4], p[5]};
        a.out[0][i] = fxk::obb_overlap(o, a.in[1] + 6 * (size_t)i) ? 1.0 : 0.0;
        break;
    }
    default: break;
    }
}
