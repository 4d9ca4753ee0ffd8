/*
 * wm_k0_power.h -- K0 channel power: the power in every pipeline row's 200 kHz channel, level block by level block (cfg.line_power).
 *
 * The band form of k0_spectrum (wm_k0_spectrum.h) leaves, for every capture and level block of a push, 32 bands of 16 bins each.
 * k0_channel_power sums, for every pipeline row r = chain x S + v, the nb bands that hold the row's channel window, and the host turns
 * that timeline into one record per datagram line: the mean over the telegram against the lower quartile of the 20 ms in front of its
 * preamble.  The arithmetic is the definition (include/wmbus_hip.h, CHANNEL POWER; tests/power_ref.py restates it): integers only,
 * every division floors.
 *
 * The kernel runs behind k0_afc_plan where there is one -- the centre of a push is known only then: it reads the held_hz that launch has
 * just committed -- otherwise behind the survey.  Shape: grid = (level blocks / 8, pipeline stream, chain), 256 threads = 8 level blocks
 * x 32 lanes, lane j reads band j of the level block's row (one coalesced 128-byte read), the lanes inside the window are summed in 64
 * bits by five xor steps, lane 0 stores.  The window's first band is the same in every thread of a block: scalar work.
 *
 * The rest of the file is host code shared with the library's entry points: the window, and the rule that makes a line's record.
 */
#ifndef WM_K0_POWER_H
#define WM_K0_POWER_H

#include <algorithm>
#include <vector>

#include "wm_k0_afc.h"

#define WM_K0_POW_BANDS     32u        /* bands of a level block, 16 bins each */
#define WM_K0_POW_WIDTH_HZ  WM_K0_AFC_WIDTH_HZ
#define WM_K0_POW_THREADS   256u
#define WM_K0_POW_SIM_HZ    325000     /* cfg.simultaneous: the T1/C1 chain lies this far above the stage's centre, the S1 chain below (wm_k1_demod.h: stgT = x e^(-j 2 pi 13 n / (32 d)), stgS its conjugate) */

/* W = clamp(floor(200000 x 512 / Fin), 1, 256), the survey's default window; nb = min(32, ceil(W / 16) + 1) bands */
struct K0PowWindow { uint32_t W, nb; };
__host__ __device__ __forceinline__ K0PowWindow k0_pow_window(uint32_t in_hz)
{
    const uint64_t w = (uint64_t)WM_K0_POW_WIDTH_HZ * WM_K0_SPEC_BINS / in_hz;
    const uint32_t W = (uint32_t)(w < 1u ? 1u : w > 256u ? 256u : w), nb = (W + 15u) / 16u + 1u;
    return K0PowWindow{W, nb > WM_K0_POW_BANDS ? WM_K0_POW_BANDS : nb};
}
/* the first band of the window centred on f Hz: cb = 256 + floor((1024 f + Fin) / (2 Fin)), lo = clamp(cb - W / 2, 0, 512 - W),
 * j0 = min(lo >> 4, 32 - nb) */
__host__ __device__ __forceinline__ uint32_t k0_pow_j0(int64_t f_hz, uint32_t in_hz, K0PowWindow w, int64_t *cb_out = nullptr, uint32_t *lo_out = nullptr)
{
    const int64_t cb = 256 + k0_afc_floor_div(1024 * f_hz + (int64_t)in_hz, 2 * (int64_t)in_hz);
    const int64_t want = cb - (int64_t)(w.W / 2u), top = (int64_t)(WM_K0_SPEC_BINS - w.W);
    const uint32_t lo = (uint32_t)(want < 0 ? 0 : want > top ? top : want);
    if (cb_out) *cb_out = cb;
    if (lo_out) *lo_out = lo;
    return (lo >> 4) < WM_K0_POW_BANDS - w.nb ? (lo >> 4) : WM_K0_POW_BANDS - w.nb;
}

struct K0PowArgs {
    const uint32_t *bands;       /* [NC][band_stride] K0SpecArgs.bands of this push                              */
    uint64_t band_stride;
    uint32_t *P;                 /* [2 S][p_stride] channel power of row chain x S + v, level block by level block */
    uint32_t p_stride;
    const K0AfcState *afc;       /* [S or NC] the state k0_afc_plan has committed for this push; NULL without AFC */
    uint32_t S, n_ch;            /* pipeline streams; channels per capture (1 without a list): capture = v / n_ch */
    uint32_t n_blk, in_hz;
    int32_t centre_hz[WM_K0_MAX_CH];     /* without AFC: cfg.input_channel_hz, or [0] = cfg.input_shift_hz         */
    int32_t chain_hz[2];         /* cfg.simultaneous: {+325000, -325000}; else 0                                  */
};

__device__ __forceinline__ uint64_t k0_pow_sum32(uint64_t v)       /* over the aligned 32 lanes of the thread */
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
        const uint32_t ol = __shfl_xor((uint32_t)v, m), oh = __shfl_xor((uint32_t)(v >> 32), m);
        v += ((uint64_t)oh << 32) | ol;
    }
    return v;
}

/* One block of WM_K0_POW_THREADS threads: blockIdx.x = eight level blocks, .y = pipeline stream v, .z = chain.  Every lane takes part in
 * every exchange; a level block past the push contributes nothing and stores nothing. */
__device__ __forceinline__ void k0_channel_power_block(const K0PowArgs &a)
{
    const uint32_t v = blockIdx.y, chain = blockIdx.z, j = threadIdx.x & 31u;
    const uint32_t blk = blockIdx.x * (WM_K0_POW_THREADS / 32u) + (threadIdx.x >> 5);
    const int64_t f = (int64_t)(a.afc ? a.afc[v].held_hz : a.centre_hz[v % a.n_ch]) + a.chain_hz[chain];
    const K0PowWindow w = k0_pow_window(a.in_hz);
    const uint32_t j0 = k0_pow_j0(f, a.in_hz, w);
    uint64_t mine = 0u;
    if (blk < a.n_blk && j >= j0 && j < j0 + w.nb) mine = a.bands[(uint64_t)(v / a.n_ch) * a.band_stride + 32u * (uint64_t)blk + j];
    const uint64_t sum = k0_pow_sum32(mine);
    if (blk < a.n_blk && j == 0u) a.P[(uint64_t)(chain * a.S + v) * a.p_stride + blk] = sum > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)sum;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(WM_K0_POW_THREADS) k0_channel_power(K0PowArgs a) { k0_channel_power_block(a); }
#endif

/* ---- host: a line's record from a row's timeline ------------------------------------------------------------------------------------ */

/* the level block of decimated sample n: m(n) = floor(n D M / L) input samples (L / M the resampler's ratio, 1 / 1 without one), >> 9 */
static inline uint64_t k0_pow_block_of(uint64_t n, uint32_t d, uint32_t L, uint32_t M)
{
    return (uint64_t)(((unsigned __int128)n * d * M / L) >> WM_K0_DC_LOG2);
}

struct K0PowRecord { uint64_t first_block; uint32_t signal, noise, ratio_q8; uint16_t n_signal, n_noise; };

/* p[0 .. n) = P of level blocks first_block .. first_block + n - 1.  A level block outside the array is missing: it is not counted. */
static inline K0PowRecord k0_line_power_rule(const uint32_t *p, uint64_t first_block, size_t n, uint64_t ka, uint64_t ke, uint32_t in_hz, std::vector<uint32_t> &scratch)
{
    K0PowRecord r{ka, 0u, 0u, 0u, 0u, 0u};
    const uint64_t G = ((uint64_t)in_hz + 51199u) / 51200u, Nn = ((uint64_t)in_hz + 25599u) / 25600u, end = first_block + n;
    /* signal: whole level blocks strictly inside the telegram */
    uint64_t s_lo = ka + 1u, s_hi = ke;                          /* [s_lo, s_hi) */
    if (s_lo < first_block) s_lo = first_block;
    if (s_hi > end) s_hi = end;
    if (s_hi > s_lo) {
        unsigned __int128 total = 0;
        for (uint64_t K = s_lo; K < s_hi; K++) total += p[K - first_block];
        const uint64_t cnt = s_hi - s_lo;
        r.signal = (uint32_t)(total / cnt);
        r.n_signal = (uint16_t)(cnt > 65535u ? 65535u : cnt);
    }
    /* noise: [ka - G - Nn, ka - G), K >= 0 */
    uint64_t n_hi = ka >= G ? ka - G : 0u, n_lo = ka >= G + Nn ? ka - G - Nn : 0u;
    if (n_lo < first_block) n_lo = first_block;
    if (n_hi > end) n_hi = end;
    if (n_hi > n_lo) {
        const size_t cnt = (size_t)(n_hi - n_lo);
        scratch.assign(p + (n_lo - first_block), p + (n_lo - first_block) + cnt);
        std::nth_element(scratch.begin(), scratch.begin() + cnt / 4u, scratch.end());
        r.noise = scratch[cnt / 4u];                             /* the element at floor(cnt / 4) of the ascending order: the lower quartile */
        r.n_noise = (uint16_t)(cnt > 65535u ? 65535u : cnt);
    }
    if (r.n_signal && r.n_noise) {
        if (r.noise == 0u) r.ratio_q8 = r.signal ? 0xFFFFFFFFu : 0u;
        else { const uint64_t q = (uint64_t)r.signal * 256u / r.noise; r.ratio_q8 = q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q; }
    }
    return r;
}

#endif
