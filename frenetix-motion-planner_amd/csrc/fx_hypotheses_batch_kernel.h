// fx_hypotheses_batch_kernel.h -- the hypotheses pass of fx_hypotheses_kernel.h for a table of ROWS in one call (DESIGN.md section
// 27; host: fx_api_hypotheses.hip; table: fx_hypotheses_batch_plan.h).
//
// A row is one agent with a contiguous range of its prediction sets: the per-agent launch's arguments (FxHypArgs) with the row's own
// pointers.  The rows of a round share each of the three launches with a flat 1-D grid; a workgroup finds its row with the ballot
// search of the other batched passes (fxrisk::batch_row_of) over the rows' first workgroups, then hypothesis, tile and chunk by
// division -- all from blockIdx alone, so the row's fields and the hypothesis' hot table stay scalar loads: the row table, like the
// tables, is written by a copy in front of the launches and by no kernel, and is read through the constant address space.  From
// there on the loops of fx_hypotheses_kernel.h in their own text (those kernels stay what they are), the partials and ballots in the
// same layout inside the row's own scratch segment.  So every result carries the bits of the per-agent call.  FP64, no atomics.
#pragma once

#include <hip/hip_runtime.h>

#include "fx_cost_sum.h"
#include "fx_hypotheses_batch_plan.h"
#include "fx_hypotheses_kernel.h"
#include "fx_risk_kernel.h"
#include "fx_select.h"

namespace fxhy {

// how the row's step summed (fx_cost_sum.h), by value
struct SumForm {
    int deferred, n_pred, n_cost;
};

// grid = all items of the round's rows: per row (hypotheses of the row) x (tiles x chunks), block = 64, dynamic LDS = CH * (largest K
// of the round's rows) * 48 B, of which a wave uses its own row's CH * K * 48 B
template <int CH>
__global__ __launch_bounds__(64, 4) void fx_hyp_batch_item_kernel(const FxHypBatchDevRow *__restrict__ rows, const int64_t *__restrict__ item0,
                                                                  const int n_rows) {
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];   // (cu, cw) [CH][K][2] | hull circles [CH][K][4]
    const auto &r = as_const(rows)[fxrisk::batch_row_of(item0, n_rows, (int64_t)blockIdx.x)];
    const auto &a = r.a;
    const int S = a.S, K = a.K, NC = a.NC;
    // (a round's items are below 2^31, so are a row's)
    const unsigned local = blockIdx.x - (unsigned)r.item0, per_hyp = (unsigned)r.items;
    const int h = (int)(local / per_hyp);
    const unsigned rest = local - (unsigned)h * per_hyp;
    const int tile = (int)(rest / (unsigned)NC), chunk = (int)(rest - (unsigned)tile * (unsigned)NC);
    const int lane = threadIdx.x & 63;
    const int64_t C = a.C, ld = a.ld;
    const int64_t c0 = (int64_t)tile * 64, c = c0 + lane;   // (c < ld: ld is C rounded up to whole tiles)
    const FX_GLOBAL uint32_t *__restrict__ flags = as_global(a.flags);
    const uint32_t f = c < C ? flags[c] : 0u;
    const bool act = (f & FX_FLAG_COSTED) != 0;
    const unsigned long long am = __builtin_amdgcn_ballot_w64(act);
    FX_GLOBAL double *__restrict__ part_out = as_global(a.part) + (((int64_t)h * NC + chunk) * ld + c);
    FX_GLOBAL unsigned long long *__restrict__ colm_out = as_global(a.colm) + (((int64_t)h * NC + chunk) * a.n_tiles + tile);
    // (every field of the row the loop needs is read here: the row's address is dead behind this prologue, and the kernel has the
    // per-agent kernel's scalar registers -- 100 / 104 / 106, two more for 2 steps per item with the fields read where they are used)
    const int n_pred = a.n_pred, col_stage = a.col_mode;
    const double ox = a.ox, oy = a.oy;
    const double wb = a.wb, half_len = a.half_len, half_wid = a.half_wid;
    const double *planes = a.planes;
    // every chunk of a tile looks at the same 64 flag words: these are tile-uniform
    const bool do_pred = n_pred >= 0 && K > 0 && am != 0ULL;
    const bool do_col = col_stage && K > 0 && fxk::wave_any_bit(act && (f & FX_FLAG_SELECTABLE));
    if (!(do_pred || do_col)) {   // nothing to add: neutral partials, so that the finish kernel reads no word nobody wrote
        *part_out = 0.0;
        if (lane == 0) *colm_out = 0ULL;
        return;
    }
    // lanes without a costed candidate walk the first costed lane's rows: every lane stays in the wave-level operations
    const int64_t g = act ? c : c0 + __builtin_ctzll(am);

    const int i_a = 1 + chunk * CH, i_b = min(S, i_a + CH);
    const int64_t ps = (int64_t)S * ld;
    const FX_GLOBAL double *__restrict__ pl = as_global(planes);
    // the hypothesis' tables: no kernel writes them -- constant address space, wave-uniform reads are scalar loads
    const FxHypTable T = fx_hyp_table(S, K);
    const size_t table_words = a.table_words;
    const double *tables = a.tables;
    const auto tab = as_const(tables) + (size_t)h * table_words;
    const auto hot_a = tab + T.hot + (size_t)i_a * K * FX_HOT_STRIDE;
    const auto rec = tab + T.rec;
    const auto pmask = reinterpret_cast<const FX_CONSTAS unsigned long long *>(tab + T.pm);
    const auto hmask = reinterpret_cast<const FX_CONSTAS unsigned long long *>(tab + T.hm);
    const double gap_margin = tab[T.margin];
    // the chunk's slice of the hot table -> LDS: per (step, obstacle) the addends (cu, cw) as one 16-byte pair, then the hull
    // circles (hx2, hy2, hr2, ck) as 32 bytes; entry e of the slice is handled by lane e, e + 64, ...
    fx_d2 *__restrict__ cc_tab = reinterpret_cast<fx_d2 *>(lds_dyn);   // [CH][K]
    double *__restrict__ circ_tab = lds_dyn + 2 * (size_t)CH * K;       // [CH][K][4]
    const int n_e = max((i_b - i_a) * K, 0);
    {
        const FX_GLOBAL double *__restrict__ hot_g = as_global(tables) + (size_t)h * table_words + T.hot + (size_t)i_a * K * FX_HOT_STRIDE;
        for (int e = lane; e < n_e; e += 64) {
            const FX_GLOBAL double *q = hot_g + (size_t)e * FX_HOT_STRIDE;
            cc_tab[e] = fx_d2{q[FX_HOT_CU], q[FX_HOT_CW]};
            circ_tab[4 * e + 0] = q[FX_HOT_HX2]; circ_tab[4 * e + 1] = q[FX_HOT_HY2]; circ_tab[4 * e + 2] = q[FX_HOT_HR2]; circ_tab[4 * e + 3] = q[FX_HOT_CK];
        }
    }
    // rows i_a - 1 .. i_b - 1 of x, y (and theta with the collision stage)
    const bool col_mode = col_stage && K > 0;
    double xs[CH + 1], ys[CH + 1], ts[CH + 1];
#pragma unroll
    for (int j = 0; j <= CH; j++) {
        const int i = min(i_a - 1 + j, S - 1);
        xs[j] = pl[(int64_t)FX_PL_X * ps + (int64_t)i * ld + g];
        ys[j] = pl[(int64_t)FX_PL_Y * ps + (int64_t)i * ld + g];
        ts[j] = col_mode ? pl[(int64_t)FX_PL_THETA * ps + (int64_t)i * ld + g] : 0.0;
    }

    double acc = 0.0;
    bool collided = false;
    {
        // constant part of a hull's bounding radius for the wave-level cull: |wb| + sqrt(2) (|wb| + hd), rounded up
        const float cull_r0 = (float)((fabs(wb) * 2.41422 + 1.41423 * sqrt(half_len * half_len + half_wid * half_wid)) * 1.00001);
        const unsigned long long full = K >= 64 ? ~0ULL : ((1ULL << K) - 1ULL);
        const int kl = min(lane, K - 1);
        // the table writes above are this wave's own: LDS operations of one wave execute in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double sn_prev = 0.0, cs_prev = 1.0;
        bool have_prev = false;   // wave-uniform: (sn_prev, cs_prev) = sin / cos of theta at step i - 1
#pragma unroll
        for (int j = 1; j <= CH; j++) {
            const int i = i_a + j - 1;
            if (i < i_b) {
                const unsigned long long pm = do_pred ? fxk::uniform_u64(pmask[i]) : 0ULL;
                const unsigned long long hm = (do_col && i >= 2) ? fxk::uniform_u64(hmask[i]) : 0ULL;
                const auto hot_i = hot_a + (size_t)(j - 1) * K * FX_HOT_STRIDE;
                const fx_d2 *__restrict__ cc_i = cc_tab + (size_t)(j - 1) * K;
                const double *__restrict__ circ_i = circ_tab + 4 * (size_t)(j - 1) * K;
                // ---- prediction cost: sum over the obstacles of 1 / m^2, fx_obstacle_body's sequence ----
                if (pm) {
                    const double xr = xs[j] - ox, yr = ys[j] - oy;
                    double ssum = 0.0;
                    auto ld_ = [&](int k) { return fxk::obs_load(hot_i, cc_i, k); };
                    if (pm == full) {
                        const int kz = K - 1;
                        ObsEntry ea = ld_(0), eb = ld_(min(1, kz)), ec, ed;
                        int k = 0;
                        for (; k + 3 < K; k += 4) {
                            ec = ld_(k + 2); ed = ld_(k + 3);
                            const double qa = fxk::obs_msq(ea, xr, yr), qb = fxk::obs_msq(eb, xr, yr);
                            ea = ld_(min(k + 4, kz)); eb = ld_(min(k + 5, kz));
                            ssum += fxk::obs_four(qa, qb, fxk::obs_msq(ec, xr, yr), fxk::obs_msq(ed, xr, yr));
                        }
                        // entries k (ea) and k + 1 (eb) are loaded where they exist; up to three remain
                        double s1 = 0.0;
                        if (k < K) ssum += fxk::rcp_pred(fxk::obs_msq(ea, xr, yr));
                        if (k + 1 < K) s1 += fxk::rcp_pred(fxk::obs_msq(eb, xr, yr));
                        if (k + 2 < K) ssum += fxk::rcp_pred(fxk::obs_msq(ld_(k + 2), xr, yr));
                        ssum += s1;
                    } else {
                        unsigned long long m = pm;
                        while (m) {
                            const int k = __builtin_ctzll(m);
                            m &= m - 1;
                            ssum += fxk::rcp_pred(fxk::obs_msq(ld_(k), xr, yr));
                        }
                    }
                    // anything not finite sends the step to the reference form on the raw records
                    if (fxk::wave_any_bit(!(ssum < 1e300))) {
                        const auto rec_i = rec + (int64_t)i * K * 12;
                        double rs = 0.0;
                        unsigned long long m = pm;
                        while (m) {
                            const int k = __builtin_ctzll(m);
                            m &= m - 1;
                            const auto q = rec_i + k * 12;
                            const double e0 = xs[j] - q[0], e1 = ys[j] - q[1];
                            const double r0 = fma(e1, q[4], e0 * q[2]), r1 = fma(e1, q[5], e0 * q[3]);
                            const double mq = fma(r1, e1, r0 * e0);
                            const double mm = mq * mq;
                            rs += mm > 0.0 ? fxk::rcp_pred(mm) : 1.0 / mm;
                        }
                        ssum = !(ssum < 1e300) ? rs : ssum;
                    }
                    acc += ssum;
                }
                // ---- collision: OBB-sum hull of ego boxes (i-1, i) against the obstacle hulls of this step ----
                if (hm) {
                    // the wave-level cull of fx_obstacle_body, in front of the headings
                    unsigned long long cand;
                    {
                        const double mxr = fma(0.5, xs[j - 1] + xs[j], -ox), myr = fma(0.5, ys[j - 1] + ys[j], -oy);
                        const double tx = xs[j] - xs[j - 1], ty = ys[j] - ys[j - 1];
                        const double qd = fma(tx, tx, ty * ty);
                        const double m0x = fxk::uniform_f64(mxr), m0y = fxk::uniform_f64(myr);
                        const double dx = mxr - m0x, dy = myr - m0y;
                        const double qe = fma(dx, dx, dy * dy);
                        const bool bad = !(qd + qe < 1e300);   // a point that is not finite keeps every obstacle on the exact path
                        const float reach = fmaf(__builtin_amdgcn_sqrtf((float)qe), 1.00001f,
                                                 fmaf(__builtin_amdgcn_sqrtf((float)qd), 0.707115f, cull_r0));
                        const unsigned rb = fxk::wave_max_u32(bad ? 0u : __float_as_uint(reach));
                        const double Rw = (double)__uint_as_float(rb);
                        const double *qo = circ_i + 4 * (size_t)kl;
                        const double ex = fma(-0.5, qo[0], -m0x), ey = fma(-0.5, qo[1], -m0y);   // h - m0
                        const double rr = fma(-0.5, qo[2], Rw) * 1.00001;                        // r_o + R
                        cand = __builtin_amdgcn_ballot_w64(!(fma(ex, ex, ey * ey) > rr * rr)) & hm;
                        if (fxk::wave_any_bit(bad)) cand = hm;
                    }
                    have_prev = have_prev && cand != 0ULL;
                    if (cand) {
                        double s0 = sn_prev, c0h = cs_prev, s1, c1;
                        if (!have_prev) fxm::sincos(ts[j - 1], &s0, &c0h);   // (wave-uniform: the previous step went the same way)
                        fxm::sincos(ts[j], &s1, &c1);
                        sn_prev = s1; cs_prev = c1;
                        const Obb hull = fxk::obb_hull(fma(wb, c0h, xs[j - 1]), fma(wb, s0, ys[j - 1]), c0h, s0, fma(wb, c1, xs[j]),
                                                       fma(wb, s1, ys[j]), c1, s1, half_len, half_wid);
                        const auto rec_i = rec + (int64_t)i * K * 12;
                        const double re = (hull.h1 + hull.h2) * 1.000001;
                        const double cxr = hull.cx - ox, cyr = hull.cy - oy;
                        const double wq = fma(cxr, cxr, fma(cyr, cyr, -re * re));
                        do {
                            const int k = __builtin_ctzll(cand);
                            cand &= cand - 1;
                            const double *q = circ_i + 4 * (size_t)k;
                            const double gq = fma(q[0], cxr, fma(q[1], cyr, fma(q[2], re, q[3] + wq)));
                            if (fxk::wave_any_bit(!(gq > gap_margin))) collided |= fxk::obb_overlap(hull, rec_i + k * 12 + 6);
                        } while (cand);
                        have_prev = true;
                    }
                } else {
                    have_prev = false;
                }
            }
        }
    }
    *part_out = acc;
    const unsigned long long cm = __builtin_amdgcn_ballot_w64(collided && act);
    if (lane == 0) *colm_out = cm;
}

// grid = all finish workgroups of the round's rows: per row (hypotheses of the row) x (tiles of FX_HYP_FINISH_TILE candidates)
__global__ __launch_bounds__(FX_HYP_FINISH_TILE) void fx_hyp_batch_finish_kernel(const FxHypBatchDevRow *__restrict__ rows,
                                                                                 const int64_t *__restrict__ fin0, const int n_rows) {
    __shared__ double sc[FX_HYP_FINISH_TILE / 64];
    __shared__ long long si[FX_HYP_FINISH_TILE / 64];
    const auto &r = as_const(rows)[fxrisk::batch_row_of(fin0, n_rows, (int64_t)blockIdx.x)];
    const auto &a = r.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t local = (int64_t)blockIdx.x - r.fin0, n_part = a.n_part;
    const int h = (int)(local / n_part), NC = a.NC;
    const int64_t blk = local - (int64_t)h * n_part;
    const int64_t c = blk * FX_HYP_FINISH_TILE + tid;
    const int64_t C = a.C, ld = a.ld;
    const bool in = c < C;
    const uint32_t f = in ? a.flags[c] : 0u;
    const bool costed = (f & FX_FLAG_COSTED) != 0, sel = (f & FX_FLAG_SELECTABLE) != 0;
    double pred = 0.0;
    unsigned long long cmask = 0ULL;
    if (in)
        for (int q = 0; q < NC; q++) {   // chunk order
            pred += a.part[((int64_t)h * NC + q) * ld + c];
            cmask |= a.colm[((int64_t)h * NC + q) * a.n_tiles + (c >> 6)];
        }
    pred = costed ? pred : 0.0;
    const bool col = sel && a.col_mode && ((cmask >> lane) & 1ULL);   // (a workgroup starts at a multiple of 64: lane == c & 63)
    const SumForm form{a.deferred, a.n_pred, a.n_cost};
    FxCostSum s;
#pragma unroll
    for (int m = 0; m < FX_NUM_COSTS; m++)
        if (m < form.n_cost) {
            const double raw = in ? a.costmap[(size_t)m * ld + c] : 0.0;
            s = fx_cost_sum_add(form, s, m, a.w[m], m == form.n_pred ? pred : raw);
        }
    s = fx_cost_sum_join(form, s);
    const double total = costed ? fx_cost_sum_total(s) : (double)NAN;
    if (in) {
        a.tot[(int64_t)h * ld + c] = total;
        a.colb[(int64_t)h * ld + c] = col ? 1 : 0;
        if (a.out_pred) a.out_pred[(int64_t)h * C + c] = pred;
        if (a.out_total) a.out_total[(int64_t)h * C + c] = total;
        if (a.out_col) a.out_col[(int64_t)h * C + c] = col ? 1 : 0;
    }
    const bool eligible = in && sel && !col && !(f & FX_FLAG_BOUNDARY) && total == total;
    double bc = eligible ? total : INFINITY;
    long long bi = eligible ? (long long)c : FX_LEX_NONE;
    fx_lex_wave_min(bc, bi);
    if (lane == 0) { sc[wave] = bc; si[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < FX_HYP_FINISH_TILE / 64; q++)
            if (fx_lex_less(sc[q], si[q], bc, bi)) { bc = sc[q]; bi = si[q]; }
        a.part_cost[(int64_t)h * n_part + blk] = bc;
        a.part_idx[(int64_t)h * n_part + blk] = bi;
    }
}

// grid = the round's (row, hypothesis) pairs, one workgroup of 1 024 lanes each
__global__ __launch_bounds__(1024) void fx_hyp_batch_select_kernel(const FxHypBatchDevRow *__restrict__ rows, const int64_t *__restrict__ sel0,
                                                                   const int n_rows) {
    __shared__ double sc[16];
    __shared__ long long si[16];
    __shared__ unsigned long long sn[16];
    const auto &r = as_const(rows)[fxrisk::batch_row_of(sel0, n_rows, (int64_t)blockIdx.x)];
    const auto &a = r.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = (int)((int64_t)blockIdx.x - r.sel0);
    const int64_t n_part = a.n_part, C = a.C, ld = a.ld;
    double bc = INFINITY;
    long long bi = FX_LEX_NONE;
    for (int64_t p = tid; p < n_part; p += 1024) {
        const double pc = a.part_cost[(int64_t)h * n_part + p];
        const long long pi = a.part_idx[(int64_t)h * n_part + p];
        if (fx_lex_less(pc, pi, bc, bi)) { bc = pc; bi = pi; }
    }
    fx_lex_wave_min(bc, bi);
    if (lane == 0) { sc[wave] = bc; si[wave] = bi; }
    __syncthreads();
    bc = sc[0]; bi = si[0];
    for (int q = 1; q < 16; q++)
        if (fx_lex_less(sc[q], si[q], bc, bi)) { bc = sc[q]; bi = si[q]; }
    const bool none = bi == FX_LEX_NONE;
    // colliding selectable candidates ordered before the winner (all of them when nothing is eligible)
    unsigned long long cnt = 0ULL;
    for (int64_t c = tid; c < C; c += 1024) {
        const uint32_t f = a.flags[c];
        const double t = a.tot[(int64_t)h * ld + c];
        if ((f & FX_FLAG_SELECTABLE) && a.colb[(int64_t)h * ld + c] && (none || t < bc || (t == bc && c < bi))) cnt++;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) sn[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long n = 0ULL;
        for (int q = 0; q < 16; q++) n += sn[q];
        a.winner[h] = none ? -1LL : bi;
        a.cost[h] = none ? (double)INFINITY : bc;
        a.n_col[h] = (long long)n;
    }
}

}  // namespace fxhy
