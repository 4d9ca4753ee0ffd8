/*
 * wm_k0_afc.h -- K0 automatic frequency correction: every capture's phase step for THIS push from its own survey (cfg.input_afc).
 *
 * k0_afc_plan sits between k0_spectrum and the stage kernel of the same push.  For every capture it evaluates the channel rule of the
 * survey (include/wmbus_hip.h, SPECTRUM: wmbus_spectrum_channels with its defaults, cap 8) on the capture's max-hold as it stands now,
 * this push's level blocks included, takes the first hit within the allowed range of the nominal, applies the hysteresis, and leaves the
 * stage kernel {step, base} of this push (K0Args.afc) and the next push the state.  The arithmetic is the definition (include/wmbus_hip.h,
 * AFC; tests/afc_ref.py restates it in Python integers); the host rule in wm_spectrum_channels.h is the oracle of the hit list.  With
 * cfg.input_spectrum_age the max-hold is the view's: the maximum of the survey's two slots, the block count their sum (SPECTRUM AGE).
 *
 * Shape: one block of 512 threads per capture (with cfg.input_channel_afc_hz: per capture and channel, the channel in blockIdx.y, each
 * with its own nominal, range and state: the early exit at the first hit in range is the block's own), thread b <-> bin b.  It is
 * latency on a context's launch chain, not throughput: one launch, the state commit inside it.
 *   Fp        rank counting: thread i counts the entries below its own (ties by index); rank 255 is the median the rule asks for
 *   windows   three inclusive prefix sums in LDS (Hillis-Steele, nine steps, ping-pong): peak, e = max(0, peak - Fp), e (b - 256); every
 *             window sum of the rule -- B[b], den, num -- is then two LDS reads, so the three re-centring trips cost thread 0 nothing
 *   argmax    key = (B << 9 | 511 - b) + 1 for a live window, 0 for a dead one: the largest B wins, the lowest b on a tie; B < 2^41.  The
 *             wave reduces with __shfl_xor (two dwords), the eight waves meet in LDS
 *   hits      at most 8 trips: thread 0 holds the hit against the thresholds, re-centres, computes offset_hz and ratio_q8 and publishes
 *             {stop, best}; every thread kills its own window if |b - best| < W.  The loop ends early at the first hit within range: the
 *             candidate is the FIRST such hit, later ones change nothing
 *   commit    thread 0: hysteresis, step, {step, base} of this push, the state of the next
 * Widths: B 256 < 2^49, min_ratio W Fp < 2^51, |num| < 2^49, 2 num + den: all inside 64 bits.  Only offset_hz = floor((2 num Fin + 512 den)
 * / (1024 den)) is wider (2 num Fin reaches 2^81): the numerator is built as two 64-bit words and divided by shift and subtract -- plain
 * 64-bit operations, the same on the device and on the block emulator of the tests, one thread, at most 8 times per push.
 */
#ifndef WM_K0_AFC_H
#define WM_K0_AFC_H

#include "wm_k0_spectrum.h"

#define WM_K0_AFC_THREADS      WM_K0_SPEC_BINS      /* a thread per bin */
#define WM_K0_AFC_WIDTH_HZ     200000u              /* the defaults of wmbus_spectrum_channels */
#define WM_K0_AFC_MIN_RATIO_Q8 1024u
#define WM_K0_AFC_REL          8u
#define WM_K0_AFC_CAP          8u
#define WM_K0_AFC_RANGE_HZ     64000u               /* cfg.input_afc_range_hz = 0 */

/* the carried state of one capture (wmbus_afc is its first four words) */
struct K0AfcState { int32_t held_hz; uint32_t locked, changes, ratio_q8, base, pad[3]; };

struct K0AfcArgs {
    const uint32_t *peak;        /* [NC][512] the survey's max-hold, this push included                        */
    const uint64_t *blocks;      /* [NC] its level blocks (0: no survey yet, no hit)                           */
    const K0AfcState *st_in;     /* [NC] the state in front of this push                                       */
    K0AfcState *st_out;          /* the same for the next push                                                 */
    K0AfcPush *push;             /* [NC] K0Args.afc                                                            */
    uint32_t in_hz;              /* Fin                                                                        */
    int32_t nominal_hz;          /* cfg.input_shift_hz                                                         */
    uint32_t range_hz;           /* a hit counts within nominal +- range                                       */
    uint32_t n_in;               /* input samples of this push                                                 */
    /* cfg.input_spectrum_age: the survey's second slot (both NULL without ageing; behind everything else: the arguments keep their places) */
    const uint32_t *peak1;       /* [NC][512] the view's max-hold is max(peak, peak1)                          */
    const uint64_t *blocks1;     /* [NC] its level blocks are blocks + blocks1                                 */
    /* cfg.input_channel_afc_hz: a lock per channel.  n_ch = 0: none, the grid is (captures), the state of block x is [x].  n_ch = C: the
     * grid is (captures, C), block (x, y) evaluates the rule on capture x's survey for channel y and owns state and push [x C + y] */
    uint32_t n_ch;
    int32_t ch_nominal_hz[WM_K0_MAX_CH];     /* cfg.input_channel_hz: take nominal_hz's place                  */
    uint32_t ch_range_hz[WM_K0_MAX_CH];      /* take range_hz's place; 0: the channel is fixed -- no search, its state never changes but for the phase */
};

/* what a block needs of LDS */
struct K0AfcLds {
    uint64_t scan[2][3][WM_K0_SPEC_BINS];            /* ping-pong: peak | e | e (b - 256), inclusive prefix sums */
    uint64_t wmax[WM_K0_AFC_THREADS / 64u];
    uint32_t pk[WM_K0_SPEC_BINS];
    uint32_t Fp, stop, best;
    int32_t cand_hz;
    uint32_t cand_ratio, found;
};

__host__ __device__ __forceinline__ int64_t k0_afc_floor_div(int64_t a, int64_t b)   /* b > 0; floors also for a < 0 */
{
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

/* floor((2 num Fin + 512 den) / (1024 den)), den > 0, |num| <= 256 den (a weighted mean of b - 256), den < 2^41: the numerator's
 * magnitude as {hi, lo}, divided by shift and subtract (the remainder stays below 1024 den < 2^51: nothing overflows); a negative
 * numerator floors as -ceil(|X| / D).  The quotient is at most (Fin + 1) / 2: it fits 32 bits. */
__host__ __device__ __forceinline__ int32_t k0_afc_offset(int64_t num, uint64_t den, uint32_t in_hz)
{
    const uint64_t a = 2u * (uint64_t)(num < 0 ? -num : num);                          /* < 2^50 */
    const uint64_t p_lo32 = (a & 0xFFFFFFFFu) * in_hz, p_hi32 = (a >> 32) * in_hz;     /* a Fin = p_hi32 2^32 + p_lo32 */
    uint64_t lo = p_lo32 + (p_hi32 << 32), hi = (p_hi32 >> 32) + (lo < p_lo32 ? 1u : 0u);
    const uint64_t half = 512u * den, D = 1024u * den;
    bool neg = false;
    if (num >= 0) { lo += half; hi += lo < half ? 1u : 0u; }
    else if (hi == 0u && lo <= half) lo = half - lo;
    else { neg = true; hi -= lo < half ? 1u : 0u; lo -= half; }
    uint64_t rem = 0u, q = 0u;
    for (int i = 127; i >= 0; i--) {
        rem = (rem << 1) | ((i >= 64 ? hi >> (i - 64) : lo >> i) & 1u);
        q <<= 1;
        if (rem >= D) { rem -= D; q |= 1u; }
    }
    return neg ? -(int32_t)(uint32_t)(q + (rem ? 1u : 0u)) : (int32_t)(uint32_t)q;
}

/* wmbus_shift_design's rule: floor((f 2^32 + Fin / 2) / Fin) mod 2^32, |f| <= Fin / 2 */
__host__ __device__ __forceinline__ uint32_t k0_afc_step(int32_t f, uint32_t in_hz)
{
    return (uint32_t)(uint64_t)k0_afc_floor_div((int64_t)f * ((int64_t)1 << 32) + (int64_t)(in_hz / 2u), (int64_t)in_hz);
}

__device__ __forceinline__ uint64_t k0_afc_wave_max(uint64_t key)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t ol = __shfl_xor((uint32_t)key, m), oh = __shfl_xor((uint32_t)(key >> 32), m);
        const uint64_t o = ((uint64_t)oh << 32) | ol;
        key = o > key ? o : key;
    }
    return key;
}

/* the sum over [i0, i0 + W) from an inclusive prefix sum (wrap-around arithmetic: also right for the signed one) */
__device__ __forceinline__ uint64_t k0_afc_window(const uint64_t *incl, uint32_t i0, uint32_t W)
{
    return incl[i0 + W - 1u] - (i0 ? incl[i0 - 1u] : 0u);
}

/* One block of WM_K0_AFC_THREADS threads: blockIdx.x = capture.  Every thread of the block arrives at every barrier. */
__device__ __forceinline__ void k0_afc_plan_block(const K0AfcArgs &a, K0AfcLds &s)
{
    constexpr uint32_t N = WM_K0_SPEC_BINS;
    const uint32_t t = threadIdx.x, cp = blockIdx.x;
    const uint32_t v = a.n_ch ? cp * a.n_ch + blockIdx.y : cp;                       /* the state's and the push's index */
    const int32_t nominal_hz = a.n_ch ? a.ch_nominal_hz[blockIdx.y] : a.nominal_hz;
    const uint32_t range_hz = a.n_ch ? a.ch_range_hz[blockIdx.y] : a.range_hz;
    const bool fixed = a.n_ch != 0u && range_hz == 0u;                               /* block-uniform */
    const uint32_t *peak = a.peak + (uint64_t)cp * N;
    uint32_t mine = peak[t];
    uint64_t blocks = a.blocks[cp];
    if (a.peak1) {                                               /* the ageing survey's view: the two slots together (SPECTRUM AGE) */
        const uint32_t other = a.peak1[(uint64_t)cp * N + t];
        mine = other > mine ? other : mine;
        blocks += a.blocks1[cp];
    }
    s.pk[t] = mine;
    if (t == 0u) { s.found = 0u; s.stop = 0u; }
    __syncthreads();
    uint32_t rank = 0u;
    for (uint32_t j = 0; j < N; j++) { const uint32_t v = s.pk[j]; rank += (v < mine || (v == mine && j < t)) ? 1u : 0u; }
    if (rank == N / 2u - 1u) s.Fp = mine ? mine : 1u;            /* sorted ascending [255]; exactly one thread has the rank */
    __syncthreads();
    const uint32_t Fp = s.Fp;
    const uint64_t e = mine > Fp ? (uint64_t)(mine - Fp) : 0u;
    s.scan[0][0][t] = mine; s.scan[0][1][t] = e; s.scan[0][2][t] = e * (uint64_t)(int64_t)((int32_t)t - 256);
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t d = 1u; d < N; d <<= 1) {
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) s.scan[cur ^ 1u][k][t] = s.scan[cur][k][t] + (t >= d ? s.scan[cur][k][t - d] : 0u);
        cur ^= 1u;
        __syncthreads();
    }
    const uint64_t *inP = s.scan[cur][0], *inE = s.scan[cur][1], *inEI = s.scan[cur][2];

    const uint64_t w_raw = (uint64_t)WM_K0_AFC_WIDTH_HZ * N / a.in_hz;
    const uint32_t W = (uint32_t)(w_raw < 1u ? 1u : w_raw > 256u ? 256u : w_raw), nB = N - W + 1u;
    const uint64_t B = t < nB ? k0_afc_window(inP, t, W) : 0u;
    bool alive = t < nB && blocks != 0u && !fixed;               /* no level block yet: the rule refuses, no hit; a fixed channel does not search */
    uint64_t first = 0u;                                         /* thread 0's */
    uint32_t hits = 0u;
    for (uint32_t trip = 0; trip < WM_K0_AFC_CAP; trip++) {
        const uint64_t key = k0_afc_wave_max(alive ? ((B << 9) | (uint64_t)(N - 1u - t)) + 1u : 0u);
        if ((t & 63u) == 0u) s.wmax[t >> 6] = key;
        __syncthreads();
        if (t == 0u) {
            uint64_t m = 0u;
            for (uint32_t w = 0; w < WM_K0_AFC_THREADS / 64u; w++) m = s.wmax[w] > m ? s.wmax[w] : m;
            const uint64_t Bb = m ? (m - 1u) >> 9 : 0u;
            const uint32_t best = m ? N - 1u - (uint32_t)((m - 1u) & (N - 1u)) : 0u;
            bool stop = m == 0u || Bb * 256u < (uint64_t)WM_K0_AFC_MIN_RATIO_Q8 * W * Fp || (hits && Bb * WM_K0_AFC_REL < first);
            if (!stop) {
                if (!hits) first = Bb;
                uint32_t lo = best;
                int64_t num = 0;
                uint64_t den = 0u;
                for (int r = 0; r < 3; r++) {
                    const uint64_t dd = k0_afc_window(inE, lo, W);
                    if (dd == 0u) break;                         /* never on the first trip (the threshold is above x 1); later: the last window stands */
                    den = dd; num = (int64_t)k0_afc_window(inEI, lo, W);
                    const int64_t cb = k0_afc_floor_div(2 * num + (int64_t)den, 2 * (int64_t)den);
                    const int64_t want = cb + 256 - (int64_t)(W / 2u);
                    const uint32_t nlo = (uint32_t)(want < 0 ? 0 : want > (int64_t)(N - W) ? (int64_t)(N - W) : want);
                    if (nlo == lo) break;
                    lo = nlo;
                }
                hits++;
                if (den != 0u) {
                    const int32_t hz = k0_afc_offset(num, den, a.in_hz);
                    const int64_t off = (int64_t)hz - (int64_t)nominal_hz;
                    if ((off < 0 ? -off : off) <= (int64_t)range_hz) {
                        const uint64_t ratio = Bb * 256u / ((uint64_t)W * Fp);
                        s.cand_hz = hz; s.cand_ratio = ratio > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ratio; s.found = 1u;
                        stop = true;                             /* the first hit within range is the candidate */
                    }
                }
            }
            s.stop = stop ? 1u : 0u; s.best = best;
        }
        __syncthreads();
        if (s.stop) break;
        const uint32_t best = s.best;
        if ((t > best ? t - best : best - t) < W) alive = false;
    }
    if (t == 0u) {
        K0AfcState st = a.st_in[v];
        if (s.found) {
            const int64_t move = (int64_t)s.cand_hz - (int64_t)st.held_hz;
            if (!st.locked || (move < 0 ? -move : move) > (int64_t)(a.in_hz / 256u)) {
                st.held_hz = s.cand_hz; st.ratio_q8 = s.cand_ratio; st.locked = 1u; st.changes++;
            }
        }
        const uint32_t step = k0_afc_step(st.held_hz, a.in_hz);
        a.push[v] = K0AfcPush{step, st.base};
        st.base += step * a.n_in;
        a.st_out[v] = st;
    }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(WM_K0_AFC_THREADS) k0_afc_plan(K0AfcArgs a)
{
    __shared__ K0AfcLds k0_afc_lds;
    k0_afc_plan_block(a, k0_afc_lds);
}
#endif

#endif
