// fx_sort_kernel.h -- the stable cost order of ALL candidates of an agent, on the device (fx_sort_candidates_*):
// what TrajectoryBundle.sort computes (trajectories.py:524-561) and PlanStepResult.sorted_ids computed on the host from 12 C bytes.
//
// A stable least-significant-digit radix sort, 8 passes of 8-bit digits, of (key, local index) pairs.  The key is the 64-bit
// order-preserving image of the cost (fx_sort_key): -0.0 first becomes +0.0 (equal in the order, the index decides), then
// sign set -> ~bits, else bits | 1 << 63; every NaN of the pool -- either sign, quiet or signalling, any payload -- gets the ONE key
// FX_SORT_KEY_NAN directly above +inf, so that NaNs come last in index order (np.argsort(kind="stable")); a candidate outside the pool
// ((flags & require) == require && (flags & exclude) == 0 fails) gets FX_SORT_KEY_OUT, all ones, and is sorted with the rest: ranks
// [0, n_pool) are the pool, no compaction runs in front.  Costs are never rebuilt from keys: the readers gather cost[order].
//
// Two decompositions (fx_launch_sort; the largest agent of the call decides):
//   * up to FX_SORT_SMALL_MAX candidates ONE workgroup sorts the agent in LDS in ONE launch (fx_sort_small_kernel): keys and indices
//     ping-pong between two LDS arrays, 24 bytes per candidate -- 96 KiB of the 160 at 4 096;
//   * above, tiles of FX_SORT_TILE keys and per pass three launches: fx_sort_hist_kernel (digit counts per tile),
//     fx_sort_scan_kernel (per agent: exclusive offsets over (digit, tile), one workgroup, the digit of a lane) and
//     fx_sort_scatter_kernel (ranks stably inside the tile and writes to the other buffer).  Pass 0 reads the cost and flag planes
//     and makes the keys on the fly, pass 7 writes the order (int64) and no keys.  No pass is skipped: which passes could be is
//     known on the device only, and a pass that conditionally does not run would make the buffer a later pass reads data-dependent.
// Stable inside a tile (and inside the small kernel's agent): wave w owns a CONTIGUOUS run of the tile, walks it in rounds of 64
// consecutive keys, and within a round the rank of a lane among the lanes with its digit is a popcount of a ballot mask below the
// lane (fx_sort_peers): waves in order, a wave's rounds in order, lanes in order.  The running count per (wave, digit) lives in LDS
// in a row that only its wave touches.
//
// No workgroup waits for another inside a kernel: every dependency between workgroups is a kernel boundary on the context's
// stream, every loop is bounded by a size known at launch (tiles, rounds, 256 digits), there is no look-back, flag, ticket or grid
// barrier.  The only atomics are non-returning LDS adds of the digit and pool counters.  Every global store is guarded by the
// agent's candidate count.  FP64 arithmetic is not involved: costs are loaded and compared as 64-bit integers.
#pragma once
#include "fx_device.h"

#define FX_SORT_BLOCK 256          // lanes of every sort workgroup (4 wave64)
#define FX_SORT_DIGIT_BITS 8
#define FX_SORT_ITEMS 8            // keys per lane of a tile
#define FX_SORT_TILE 2048          // keys per tile of the general decomposition
#define FX_SORT_SMALL_MAX 4096     // largest agent the one-workgroup kernel takes
#define FX_SORT_DIGITS (1 << FX_SORT_DIGIT_BITS)
#define FX_SORT_PASSES (64 / FX_SORT_DIGIT_BITS)
#define FX_SORT_WAVES (FX_SORT_BLOCK / 64)
#define FX_SORT_KEY_NAN 0xFFF0000000000001ULL
#define FX_SORT_KEY_OUT 0xFFFFFFFFFFFFFFFFULL
static_assert(FX_SORT_TILE == FX_SORT_BLOCK * FX_SORT_ITEMS, "a tile is FX_SORT_ITEMS keys per lane");
static_assert(FX_SORT_DIGITS == FX_SORT_BLOCK, "one lane per digit in the offset steps");
// LDS of the one-workgroup kernel for an agent of n candidates: two key and two index arrays over the padded count, the
// (wave, digit) counters, the waves' scan sums and the two pool counters
#define FX_SORT_SMALL_PAD(n) ((((n) + FX_SORT_BLOCK - 1) / FX_SORT_BLOCK) * FX_SORT_BLOCK)
#define FX_SORT_SMALL_LDS(n) ((size_t)FX_SORT_SMALL_PAD(n) * 24 + sizeof(uint32_t) * (FX_SORT_WAVES * FX_SORT_DIGITS + 8))

#ifndef FX_SORT_DEFINES_ONLY   // (fx_api_sort.hip sizes its buffers by the #defines above and compiles no kernel)

__device__ __forceinline__ unsigned long long fx_sort_key(unsigned long long bits, uint32_t flags, uint32_t require, uint32_t exclude,
                                                           bool *pool, bool *nan) {
    const bool in = (flags & require) == require && (flags & exclude) == 0u;
    const bool is_nan = (bits & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL;
    if (bits == 0x8000000000000000ULL) bits = 0ULL;
    unsigned long long k = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
    if (is_nan) k = FX_SORT_KEY_NAN;
    if (!in) k = FX_SORT_KEY_OUT;
    *pool = in;
    *nan = in && is_nan;
    return k;
}

// the active lanes of the wave whose digit equals the caller's (every lane of the wave calls this: 9 ballots)
__device__ __forceinline__ unsigned long long fx_sort_peers(uint32_t digit, bool active) {
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int b = 0; b < FX_SORT_DIGIT_BITS; b++) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// exclusive prefix sum of one value per lane over the workgroup's 256 lanes; wsum: FX_SORT_WAVES words of LDS
__device__ __forceinline__ uint32_t fx_sort_block_excl(uint32_t v, uint32_t *wsum) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < FX_SORT_WAVES; k++)
        if (k < w) base += wsum[k];
    __syncthreads();
    return base + inc - v;
}

// One round of a wave's stable ranking: the rank of the lane's key among the keys of its digit that this wave has seen so far, and
// the counter row `cnt` (this wave's, FX_SORT_DIGITS words of LDS) moved on by the round.  Only this wave touches the row; its LDS
// operations are issued and completed in program order, the volatile accesses and the wave barriers keep the compiler from moving
// the next round's read above this round's write.
__device__ __forceinline__ uint32_t fx_sort_round(volatile uint32_t *cnt, uint32_t digit, bool active) {
    const int lane = (int)threadIdx.x & 63;
    const unsigned long long peers = fx_sort_peers(digit, active);
    const uint32_t below = (uint32_t)__popcll(peers & ((1ULL << lane) - 1ULL));
    const uint32_t prev = active ? cnt[digit] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (active && below == 0u) cnt[digit] = prev + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    return prev + below;
}

// ---- one workgroup, one launch: agents of at most FX_SORT_SMALL_MAX candidates ----
__global__ __launch_bounds__(FX_SORT_BLOCK) void fx_sort_small_kernel(const FxSortArgs a) {
    extern __shared__ unsigned long long fx_sort_lds[];
    const int ag = a.agent0 + (int)blockIdx.y;
    const FxSortAgent A = a.agents[ag];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = (int)(A.C < FX_SORT_SMALL_MAX ? A.C : FX_SORT_SMALL_MAX);
    const int n_pad = FX_SORT_SMALL_PAD(n), per = n_pad / FX_SORT_BLOCK;   // rounds of a wave
    unsigned long long *key0 = fx_sort_lds, *key1 = key0 + n_pad;
    uint32_t *idx0 = reinterpret_cast<uint32_t *>(key1 + n_pad), *idx1 = idx0 + n_pad;
    uint32_t *cnt = idx1 + n_pad, *wsum = cnt + FX_SORT_WAVES * FX_SORT_DIGITS, *red = wsum + 4;
    const FX_GLOBAL unsigned long long *cost = reinterpret_cast<const FX_GLOBAL unsigned long long *>(as_global(A.cost));
    const FX_GLOBAL uint32_t *flags = as_global(A.flags);

    if (tid < 2) red[tid] = 0u;
    __syncthreads();
    uint32_t n_in = 0, n_nan = 0;
    for (int i = tid; i < n_pad; i += FX_SORT_BLOCK) {
        unsigned long long k = FX_SORT_KEY_OUT;   // (the padding sorts behind every candidate: same key as one outside the pool, higher index)
        if (i < n) {
            bool in, nan;
            k = fx_sort_key(cost[i], flags[i], a.require, a.exclude, &in, &nan);
            n_in += in; n_nan += nan;
        }
        key0[i] = k;
        idx0[i] = (uint32_t)i;
    }
    if (n_in) atomicAdd(&red[0], n_in);
    if (n_nan) atomicAdd(&red[1], n_nan);
    __syncthreads();
    if (tid < 2) a.counts[2 * ag + tid] = (int64_t)red[tid];

    const int first = w * per * 64;   // the wave's run of the agent
    for (int pass = 0; pass < FX_SORT_PASSES; pass++) {
        const unsigned long long *ks = (pass & 1) ? key1 : key0;
        unsigned long long *kd = (pass & 1) ? key0 : key1;
        const uint32_t *is = (pass & 1) ? idx1 : idx0;
        uint32_t *id = (pass & 1) ? idx0 : idx1;
        const int shift = pass * FX_SORT_DIGIT_BITS;
#pragma unroll
        for (int k = 0; k < FX_SORT_WAVES; k++) cnt[k * FX_SORT_DIGITS + tid] = 0u;
        __syncthreads();
        for (int r = 0; r < per; r++) {
            const uint32_t d = (uint32_t)(ks[first + r * 64 + lane] >> shift) & (FX_SORT_DIGITS - 1);
            atomicAdd(&cnt[w * FX_SORT_DIGITS + d], 1u);
        }
        __syncthreads();
        // first rank of (wave, digit): the digits in front, then the waves in front
        uint32_t c[FX_SORT_WAVES], tot = 0;
#pragma unroll
        for (int k = 0; k < FX_SORT_WAVES; k++) { c[k] = cnt[k * FX_SORT_DIGITS + tid]; tot += c[k]; }
        uint32_t at = fx_sort_block_excl(tot, wsum);
#pragma unroll
        for (int k = 0; k < FX_SORT_WAVES; k++) { cnt[k * FX_SORT_DIGITS + tid] = at; at += c[k]; }
        __syncthreads();
        for (int r = 0; r < per; r++) {
            const int i = first + r * 64 + lane;
            const unsigned long long k = ks[i];
            const uint32_t v = is[i];
            const uint32_t d = (uint32_t)(k >> shift) & (FX_SORT_DIGITS - 1);
            const uint32_t pos = fx_sort_round(cnt + w * FX_SORT_DIGITS, d, true);
            if (pass == FX_SORT_PASSES - 1) {
                if (pos < (uint32_t)n) as_global(a.order)[A.off + pos] = (int64_t)v;
            } else if (pos < (uint32_t)n_pad) {
                kd[pos] = k;
                id[pos] = v;
            }
        }
        __syncthreads();
    }
}

// ---- the general decomposition ----
// key and local index of candidate i of the agent in pass `FIRST ? 0 : later`
template <bool FIRST>
__device__ __forceinline__ unsigned long long fx_sort_load(const FxSortArgs &a, const FxSortAgent &A, int src, int64_t i, uint32_t *v, bool *in,
                                                            bool *nan) {
    if (FIRST) {
        *v = (uint32_t)i;
        return fx_sort_key(reinterpret_cast<const FX_GLOBAL unsigned long long *>(as_global(A.cost))[i], as_global(A.flags)[i], a.require,
                           a.exclude, in, nan);
    }
    *v = as_global(a.idx[src])[A.off + i];
    *in = *nan = false;
    return as_global(a.key[src])[A.off + i];
}

// digit counts of every tile; in pass 0 the tile's pool and NaN counts too
template <bool FIRST>
__global__ __launch_bounds__(FX_SORT_BLOCK) void fx_sort_hist_kernel(const FxSortArgs a, int pass) {
    __shared__ uint32_t h[FX_SORT_DIGITS + 2];
    const int ag = a.agent0 + (int)blockIdx.y, tid = (int)threadIdx.x;
    const FxSortAgent A = a.agents[ag];
    const int64_t base = (int64_t)blockIdx.x * FX_SORT_TILE;
    if (base >= A.C) return;   // (the whole workgroup: agents smaller than the call's largest)
    h[tid] = 0u;
    if (tid < 2) h[FX_SORT_DIGITS + tid] = 0u;
    __syncthreads();
    const int src = (pass & 1) ^ 1, shift = pass * FX_SORT_DIGIT_BITS;   // pass p reads what pass p - 1 wrote: buffer (p - 1) & 1
    uint32_t n_in = 0, n_nan = 0;
#pragma unroll
    for (int u = 0; u < FX_SORT_ITEMS; u++) {
        const int64_t i = base + u * FX_SORT_BLOCK + tid;
        if (i < A.C) {
            uint32_t v;
            bool in, nan;
            const unsigned long long k = fx_sort_load<FIRST>(a, A, src, i, &v, &in, &nan);
            atomicAdd(&h[(uint32_t)(k >> shift) & (FX_SORT_DIGITS - 1)], 1u);
            n_in += in; n_nan += nan;
        }
    }
    if (FIRST) {
        if (n_in) atomicAdd(&h[FX_SORT_DIGITS], n_in);
        if (n_nan) atomicAdd(&h[FX_SORT_DIGITS + 1], n_nan);
    }
    __syncthreads();
    const size_t row = (size_t)ag * a.tiles_max + blockIdx.x;
    as_global(a.hist)[row * FX_SORT_DIGITS + tid] = h[tid];
    if (FIRST && tid < 2) as_global(a.tcount)[row * 2 + tid] = h[FX_SORT_DIGITS + tid];
}

// per agent: counts of (tile, digit) -> ranks in front of the tile within the digit; dbase[digit] = ranks in front of the digit.
// Lane = digit: a tile's row of 256 counts is one coalesced access.
template <bool FIRST>
__global__ __launch_bounds__(FX_SORT_BLOCK) void fx_sort_scan_kernel(const FxSortArgs a) {
    __shared__ uint32_t wsum[FX_SORT_WAVES];
    const int ag = a.agent0 + (int)blockIdx.y, tid = (int)threadIdx.x;
    const FxSortAgent A = a.agents[ag];
    int n_tiles = (int)((A.C + FX_SORT_TILE - 1) / FX_SORT_TILE);
    if (n_tiles > a.tiles_max) n_tiles = a.tiles_max;
    FX_GLOBAL uint32_t *h = as_global(a.hist) + (size_t)ag * a.tiles_max * FX_SORT_DIGITS;
    uint32_t run = 0;
    for (int t = 0; t < n_tiles; t++) {
        const uint32_t v = h[(size_t)t * FX_SORT_DIGITS + tid];
        h[(size_t)t * FX_SORT_DIGITS + tid] = run;
        run += v;
    }
    as_global(a.dbase)[(size_t)ag * FX_SORT_DIGITS + tid] = fx_sort_block_excl(run, wsum);
    if (FIRST && tid < 2) {
        const FX_GLOBAL uint32_t *tc = as_global(a.tcount) + (size_t)ag * a.tiles_max * 2;
        int64_t s = 0;
        for (int t = 0; t < n_tiles; t++) s += tc[(size_t)t * 2 + tid];
        as_global(a.counts)[2 * ag + tid] = s;
    }
}

// a tile's keys to their ranks in the other buffer.  Wave w owns keys [512 w, 512 w + 512) of the tile, lane l the keys l, 64 + l, ...
// of that run: eight rounds of 64 consecutive keys.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(FX_SORT_BLOCK) void fx_sort_scatter_kernel(const FxSortArgs a, int pass) {
    __shared__ uint32_t cnt[FX_SORT_WAVES * FX_SORT_DIGITS];
    const int ag = a.agent0 + (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const FxSortAgent A = a.agents[ag];
    const int64_t base = (int64_t)blockIdx.x * FX_SORT_TILE;
    if (base >= A.C) return;
#pragma unroll
    for (int k = 0; k < FX_SORT_WAVES; k++) cnt[k * FX_SORT_DIGITS + tid] = 0u;
    __syncthreads();
    const int src = (pass & 1) ^ 1, dst = pass & 1, shift = pass * FX_SORT_DIGIT_BITS;
    unsigned long long key[FX_SORT_ITEMS];
    uint32_t val[FX_SORT_ITEMS], rank[FX_SORT_ITEMS];
#pragma unroll
    for (int u = 0; u < FX_SORT_ITEMS; u++) {
        const int64_t i = base + w * (FX_SORT_ITEMS * 64) + u * 64 + lane;
        key[u] = FX_SORT_KEY_OUT;
        val[u] = 0u;
        bool in, nan;
        if (i < A.C) key[u] = fx_sort_load<FIRST>(a, A, src, i, &val[u], &in, &nan);
    }
#pragma unroll
    for (int u = 0; u < FX_SORT_ITEMS; u++) {
        const int64_t i = base + w * (FX_SORT_ITEMS * 64) + u * 64 + lane;
        rank[u] = fx_sort_round(cnt + w * FX_SORT_DIGITS, (uint32_t)(key[u] >> shift) & (FX_SORT_DIGITS - 1), i < A.C);
    }
    __syncthreads();
    {   // first rank of (wave, digit): ranks in front of the digit, of the tile within it, of the wave within the tile
        const size_t row = (size_t)ag * a.tiles_max + blockIdx.x;
        uint32_t at = as_global(a.dbase)[(size_t)ag * FX_SORT_DIGITS + tid] + as_global(a.hist)[row * FX_SORT_DIGITS + tid];
#pragma unroll
        for (int k = 0; k < FX_SORT_WAVES; k++) {
            const uint32_t ck = cnt[k * FX_SORT_DIGITS + tid];
            cnt[k * FX_SORT_DIGITS + tid] = at;
            at += ck;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FX_SORT_ITEMS; u++) {
        const int64_t i = base + w * (FX_SORT_ITEMS * 64) + u * 64 + lane;
        if (i < A.C) {
            const int64_t pos = (int64_t)cnt[w * FX_SORT_DIGITS + ((uint32_t)(key[u] >> shift) & (FX_SORT_DIGITS - 1))] + rank[u];
            if (pos < A.C) {   // (always, with consistent counts: no store leaves the agent's segment whatever the counts say)
                if (LAST) {
                    as_global(a.order)[A.off + pos] = (int64_t)val[u];
                } else {
                    as_global(a.key[dst])[A.off + pos] = key[u];
                    as_global(a.idx[dst])[A.off + pos] = val[u];
                }
            }
        }
    }
}

// cost and flag word of ranks [0, n) of `order` (already offset to the first rank wanted), gathered from the agent's planes:
// the bits as they were written, NaN payloads and the sign of zero included
__global__ __launch_bounds__(FX_SORT_BLOCK) void fx_sort_gather_kernel(const int64_t *__restrict__ order, int64_t n, const double *cost,
                                                                       const uint32_t *flags, int64_t C, unsigned long long *out_cost,
                                                                       uint32_t *out_flags) {
    const int64_t j = (int64_t)blockIdx.x * FX_SORT_BLOCK + threadIdx.x;
    if (j >= n) return;
    const int64_t l = order[j];
    const bool ok = l >= 0 && l < C;
    if (out_cost) out_cost[j] = ok ? reinterpret_cast<const FX_GLOBAL unsigned long long *>(as_global(cost))[l] : 0ULL;
    if (out_flags) out_flags[j] = ok ? as_global(flags)[l] : 0u;
}

#endif  // FX_SORT_DEFINES_ONLY
