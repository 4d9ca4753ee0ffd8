/* wm_k3_levels.h -- cfg.line_levels: the frequency offset and the deviation of every telegram candidate, measured on the soft symbols
 * of the preamble in front of its access code (the arithmetic: include/wmbus_hip.h, LINE LEVELS; tests/level_ref.py restates it), and
 * the soft-symbol tail a context carries from push to push for it.  Device code, included by wm_kernels.hip behind wm_k3_bursts.h. */
#ifndef WM_K3_LEVELS_H
#define WM_K3_LEVELS_H

#define WM_LEV_TAIL   782u         /* soft symbols carried per (chain, capture): the longest reach of a window in front of its access code */
#define WM_LEV_LO_T   256u         /* T1/C1 chain: the window is [a - 256, a - 128), 16 chips of 8 samples */
#define WM_LEV_HI_T   128u
#define WM_LEV_LO_S   782u         /* S1 chain: [a - 782, a - 586), 196 samples = 8 chips of 24.4 */
#define WM_LEV_HI_S   586u
#define WM_LEV_SCALE  1048576.0f   /* 2^20 units per unit of soft symbol */
#define WM_LEV_QMAX   1048576

#include "../../include/wmbus_hip.h"
typedef wmbus_level WmLevel;     /* the kernel writes the very records wmbus_line_levels() hands out */

struct K3LevArgs {
    WmPush g;
    const float *dphi;           /* [2][S][Mcap] this push's soft symbols */
    const float *tail_in;        /* [2 S][WM_LEV_TAIL] the soft symbols in front of this push, oldest first (zero before the stream) */
    float *tail_out;             /* the same for the next push */
    /* what k3_bursts has just left beside its records (K3Args.lev_pkt / lev_hdr): {access-code sample within the push, row} per slot */
    const uint2 *src_pkts; const uint32_t *n_pkts; uint32_t pkts_cap;      /* src_pkts == nullptr: every burst is a header */
    const uint2 *src_hdr; const uint32_t *n_hdr; uint32_t hdr_cap;
    WmLevel *lev_pkts, *lev_hdr; /* [pkts_cap], [hdr_cap] pinned host memory: record i belongs to packet / header i */
};

/* q = clamp(rint(s 2^20), -2^20, 2^20): the product is exact, rintf is the hardware's round-to-nearest-even, NaN -> 0 */
__device__ __forceinline__ int32_t lev_quant(float s)
{
    float v = rintf(s * WM_LEV_SCALE);
    v = v < -WM_LEV_SCALE ? -WM_LEV_SCALE : v > WM_LEV_SCALE ? WM_LEV_SCALE : v;       /* a NaN fails both comparisons */
    return v == v ? (int32_t)v : 0;
}

__device__ __forceinline__ int64_t lev_floordiv(int64_t a, int64_t b)      /* b > 0 */
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}

__device__ __forceinline__ int32_t lev_wave_sum(int32_t v)
{
    uint32_t u = (uint32_t)v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) u += __shfl_xor(u, off);
    return (int32_t)u;
}

/* One record (packet slot r for r < np, else header slot r - np), by one wave. */
__device__ void level_item(const K3LevArgs &a, const uint32_t r, const uint32_t np, const uint32_t ln)
{
    const WmPush &g = a.g;
    const uint2 src = r < np ? a.src_pkts[r] : a.src_hdr[r - np];
    WmLevel *out = r < np ? a.lev_pkts + r : a.lev_hdr + (r - np);
    /* a continuation (~0) was measured in the push that held its access code */
    const uint32_t rel = src.y < 2u * g.S ? src.x : 0xFFFFFFFFu, ch = src.y / g.S;      /* rel: the access-code chip's sample within the push */
    WmLevel lv = {};
    if (rel < g.M) {
        const uint32_t lo = ch ? WM_LEV_LO_S : WM_LEV_LO_T, hi = ch ? WM_LEV_HI_S : WM_LEV_HI_T, N = lo - hi;
        const uint64_t sync = g.m0 + rel;
        lv.sync_sample = sync;
        if (sync >= lo) {
            const uint64_t row = src.y;
            const float *now = a.dphi + row * g.Mcap, *before = a.tail_in + row * WM_LEV_TAIL + WM_LEV_TAIL;
            const int32_t w0 = (int32_t)rel - (int32_t)lo;           /* first sample of the window, relative to the push: >= -WM_LEV_TAIL */
            int32_t q[4], sum = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {                            /* N <= 196 < 4 x 64: lane-contiguous loads, the values stay in registers */
                const uint32_t j = ln + 64u * (uint32_t)t;
                q[t] = 0;
                if (j < N) { const int32_t m = w0 + (int32_t)j; q[t] = lev_quant(m >= 0 ? now[m] : before[m]); }
                sum += q[t];
            }
            sum = lev_wave_sum(sum);
            const int32_t mean = (int32_t)lev_floordiv(2 * (int64_t)sum + N, 2 * (int64_t)N);
            int32_t adev = 0;
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (ln + 64u * (uint32_t)t < N) adev += q[t] >= mean ? q[t] - mean : mean - q[t];
            adev = lev_wave_sum(adev);                               /* <= 196 x 2^21 < 2^31 */
            lv.offset_hz = (int32_t)lev_floordiv((int64_t)sum * 3125 + (int64_t)N * 4096, (int64_t)N * 8192);
            lv.dev_hz = (uint32_t)lev_floordiv((int64_t)adev * 3125 + (int64_t)N * 4096, (int64_t)N * 8192);
            lv.n = N;
        }
    }
    if (ln == 0) *out = lv;
}

/* Behind k3_bursts, on its records: as few blocks as that kernel, for the same reason. */
__global__ __launch_bounds__(256) void k3_levels(K3LevArgs a)
{
    wm_framer_prio();
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t np = a.src_pkts ? min(*a.n_pkts, a.pkts_cap) : 0u, nh = min(*a.n_hdr, a.hdr_cap);
    for (uint32_t r = blockIdx.x * 4u + wv; r < np + nh; r += gridDim.x * 4u) level_item(a, r, np, ln);
}

/* The tail for the next push: the last WM_LEV_TAIL soft symbols of (old tail ++ this push), whatever the push's length.
 * grid (ceil(WM_LEV_TAIL / 256), 2 S). */
__global__ __launch_bounds__(256) void k3_level_tail(K3LevArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, row = blockIdx.y;
    if (i >= WM_LEV_TAIL) return;
    const int64_t m = (int64_t)a.g.M - (int64_t)WM_LEV_TAIL + i;     /* sample of the push, or (negative) of the old tail */
    a.tail_out[(uint64_t)row * WM_LEV_TAIL + i] = m >= 0 ? a.dphi[(uint64_t)row * a.g.Mcap + m] : a.tail_in[(uint64_t)row * WM_LEV_TAIL + (uint32_t)(m + WM_LEV_TAIL)];
}

#endif /* WM_K3_LEVELS_H */
