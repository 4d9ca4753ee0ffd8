/*
 * wm_k0_spectrum.h -- K0 survey: the integer max-hold spectrum of every capture (cfg.input_spectrum).
 *
 * For every capture and every level block of 512 input samples a 512-point Hann-windowed DFT in exact integers; per capture and bin the
 * sum of the power and its maximum, accumulated over the pushes of a context.  The stage only READS the raw input (in front of the
 * rotation, the resampler and the gain; behind the DC blocker's table where there is one): the bytes the pipeline gets do not change.
 *
 * The arithmetic is the definition (include/wmbus_hip.h, SPECTRUM; tests/spectrum_ref.py restates it in numpy):
 *   v = 64 x' (cu8 / cs8) or x' (cs16 / cf32);  w[n] = (16384 - c[2 n] + 1) >> 1;  y = (v w + 8192) >> 14
 *   z = y in bit-reversed order, nine radix-2 decimation-in-time stages, t = b e^(-j 2 pi i / 1024) from the shift's {c, s} table with the
 *   rotation's rounding, z = a +- t in int32;  pw = (re^2 + im^2) >> 16;  bin (j + 256) mod 512;  sum += pw, peak = max(peak, pw).
 * The butterfly graph and its roundings are the contract, the schedule below is not.
 *
 * Shape: grid = (runs of K0SpecArgs.run consecutive level blocks, capture), one WAVE per run, four waves per block, each with 2 x 576
 * dwords of LDS of its own; the waves of a block never meet (no __syncthreads: a wave whose run lies past the push leaves alone).  A lane
 * owns 8 of the 512 points throughout:
 *   load      16 raw bytes per lane and load (1 / 1 / 2 / 4 loads for cu8 / cs8 / cs16 / cf32), consecutive lanes consecutive memory;
 *             the window of the lane's 8 samples sits in registers for the whole run; y, a pair of int16, goes to LDS
 *   pass 0    points 8 L + q (bit-reversed sample order), stages 1-3: twiddles 0, 128, 256, 384 -- entries 0 and 256 multiply exactly
 *             (t = b, t = {b_im, -b_re}), so only two of the twelve butterflies multiply
 *   pass 1    points hi 64 + q 8 + lo, lane = {hi, lo}, stages 4-6;   pass 2   points q 64 + L, stages 7-9
 *   between the passes re and im cross the wave through LDS at index p + (p >> 3): ds_write_b32 / ds_read_b32 bank on (address / 4) mod 32
 *   per 32-lane half, and the padding makes the stride-8 accesses of pass 0 (9 L + q) and the {hi, lo} accesses of pass 1 (hi 72 + lo)
 *   conflict free; pass 2 (mid 9 + lo) keeps three two-way conflicts per half
 *   A lane's seven twiddles of pass 1 and of pass 2 are loop invariants: in registers for the run.
 * The 40-bit twiddle products are 64-bit multiply-adds (V_MAD_I64_I32).  The form without them -- b = bh 1024 + bl, two V_DOT2_I32_I16 per
 * half and component, (A + (B >> 10)) >> 4, bit for bit the same integers -- was built first and measured slower (DESIGN.md section 6:
 * 0.78 against 0.61 ms per push of 64 x 2^22 samples); it is gone.
 * sum (uint64) and peak of the lane's 8 bins stay in registers over the run; at its end one 64-bit
 * atomic add and one 32-bit atomic max per bin (consecutive lanes, consecutive bins) and one add to the capture's block count.
 *
 * The survey that forgets (cfg.input_spectrum_age = A, include/wmbus_hip.h, SPECTRUM AGE; tests/afc_age_ref.py): level block K of the
 * stream (64 bits, counted over all pushes) belongs to epoch K >> A and accumulates into slot (K >> A) & 1 of two sets of accumulators;
 * the view is the two slots together, the last two epochs.  The HOST decides what a push clears and what it skips (k0_spec_age_plan
 * below: the one owner of that decision, shared with the emulator harness of the tests); the AGE form of the kernel leaves out the level
 * blocks of epochs below e_keep -- a prefix of the push, not transformed at all -- and flushes its registers whenever the epoch changes
 * inside a wave's run, and at its end, with the same atomics.  AGE = false is the code above.
 *
 * The band form (cfg.line_power, include/wmbus_hip.h, CHANNEL POWER; tests/power_ref.py): BANDS = true keeps the time axis, coarsely.  At
 * the end of a level block a lane holds pw of bins 64 (q ^ 4) + lane, q = 0 .. 7: a band of 16 bins is 16 consecutive lanes of one q, a
 * DPP row.  Each row is summed in 64 bits in four steps (quad_perm 1 0 3 2, quad_perm 2 3 0 1, row_half_mirror, row_mirror: after every
 * step the partners hold the same sum, so the mirrors reach the other half as the xor would), clamped to 32 bits, and lane q of every
 * row keeps q's value: ONE store of 32 lanes writes the level block's 32 bands, a contiguous 128-byte row of K0SpecArgs.bands.  No LDS,
 * no atomics.  With AGE every level block of the push is transformed and written -- the prefix of old epochs too -- and only the
 * accumulation into the slots keeps skipping it.  BANDS = false is the code above.
 */
#ifndef WM_K0_SPECTRUM_H
#define WM_K0_SPECTRUM_H

#include "wm_k0_resample.h"

#define WM_K0_SPEC_BINS  512u      /* = one level block (WM_K0_DC_LOG2) */
#define WM_K0_SPEC_PLANE 576u      /* dwords of one LDS plane: index p + (p >> 3), p < 512 */
#define WM_K0_SPEC_WAVES 4u        /* waves (runs) per block */

#ifndef WM_K0_WAVE_SYNC            /* LDS hand-over inside one wave: its DS operations are in order, the compiler must keep them so */
#define WM_K0_WAVE_SYNC() (__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"), __builtin_amdgcn_wave_barrier())
#endif

struct K0SpecArgs {
    const uint8_t *raw;          /* [NC][raw_stride] the raw bytes of this push                                */
    uint64_t raw_stride;
    const uint32_t *dc_tab;      /* [NC][dc_stride] K0Args.dc_tab (the DC instantiations only)                 */
    uint32_t dc_stride;
    const uint32_t *shift_tab;   /* [1024] {c, s} int16: the shift's table                                     */
    uint64_t *sum;               /* [NC][512] += power per bin, bin b <-> (b - 256) Fin / 512                   */
    uint32_t *peak;              /* [NC][512] max-hold                                                          */
    uint64_t *blocks;            /* [NC] += level blocks                                                        */
    uint32_t n_blk, run;         /* level blocks of this push per capture; consecutive level blocks per wave    */
    /* the AGE form only (behind everything else: the plain form's arguments keep their places) */
    uint32_t age;                /* A: 2^A level blocks per epoch                                               */
    uint64_t k_first;            /* the stream's index of this push's first level block                        */
    uint64_t e_keep;             /* level blocks of epochs below this one are left out                         */
    uint64_t slot_stride;        /* slot 1 of sum / blocks lies this many uint64 behind slot 0, of peak twice as many uint32 */
    /* the band form only (behind everything else again) */
    uint32_t *bands;             /* [NC][band_stride] level block `blk` of the push: 32 uint32 at 32 blk, band j = bins [16 j, 16 j + 16) */
    uint64_t band_stride;
};

/* What a push of n_blk > 0 level blocks, the first of them the stream's k_first, does to the two slots of an ageing survey.  The push
 * ends in epoch e_now = (k_first + n_blk - 1) >> age; the level block in front of it lay in e_prev (none for k_first = 0, where every
 * slot is still clear).  Every epoch in (e_prev, e_now] is newly entered: one of them -- its slot still holds epoch e_now - 2: clear it;
 * two or more -- neither slot holds anything of e_now - 1 or e_now: clear both.  Level blocks of epochs below e_keep = e_now - 1 have
 * no place in the view: the kernel leaves them out. */
struct K0SpecAgePlan { uint64_t e_keep; uint32_t clear; };       /* clear: bit s set <-> slot s is zeroed in front of the kernel */
__host__ __device__ __forceinline__ K0SpecAgePlan k0_spec_age_plan(uint64_t k_first, uint32_t n_blk, uint32_t age)
{
    const uint64_t e_now = (k_first + n_blk - 1u) >> age;
    const uint64_t entered = k_first ? e_now - ((k_first - 1u) >> age) : 0u;
    return K0SpecAgePlan{e_now ? e_now - 1u : 0u, entered == 0u ? 0u : entered == 1u ? 1u << (e_now & 1u) : 3u};
}

__device__ __forceinline__ void k0_add64(uint64_t *p, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd((unsigned long long *)p, (unsigned long long)v);
#else
    *p += v;                                                     /* the block emulator runs one lane at a time */
#endif
}
__device__ __forceinline__ void k0_max32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}

__device__ __forceinline__ uint32_t k0_spec_pad(uint32_t p) { return p + (p >> 3); }

/* t = b e^(-j 2 pi i / 1024), cs = {c, s} of entry i: t_re = (b_re c + b_im s + 8192) >> 14, t_im = (b_im c - b_re s + 8192) >> 14, the
 * products 40 bits wide: the rule as it is written, two V_MAD_I64_I32 per component and a funnel shift. */
__device__ __forceinline__ void k0_spec_twiddle(int32_t br, int32_t bi, uint32_t cs, int32_t &tr, int32_t &ti)
{
    const int64_t c = (int16_t)(cs & 0xFFFFu), s = (int16_t)(cs >> 16);
    tr = (int32_t)(((int64_t)br * c + (int64_t)bi * s + 8192) >> 14);
    ti = (int32_t)(((int64_t)bi * c - (int64_t)br * s + 8192) >> 14);
}

/* three radix-2 stages on the lane's 8 points.  tw: the twiddles of local stage 0 | 1 | 2 = [1] | [2] | [4] entries {c, s}; FIRST: pass 0,
 * whose twiddles are the table's entries 0 | 0, 256 | 0, 128, 256, 384 in every lane (0 and 256 multiply exactly: done without) */
template <bool FIRST> __device__ __forceinline__ void k0_spec_pass(int32_t (&zr)[8], int32_t (&zi)[8], const uint32_t (&tw)[7])
{
#pragma unroll
    for (uint32_t t = 0; t < 3u; t++) {
        const uint32_t half = 1u << t;
#pragma unroll
        for (uint32_t g = 0; g < 8u; g += 2u * half) {
#pragma unroll
            for (uint32_t j = 0; j < half; j++) {
                const uint32_t ia = g + j, ib = g + j + half;
                int32_t tr, ti;
                if (FIRST && j * (4u >> t) == 0u) { tr = zr[ib]; ti = zi[ib]; }                       /* entry 0 = {16384, 0} */
                else if (FIRST && j * (4u >> t) == 2u) { tr = zi[ib]; ti = -zr[ib]; }                 /* entry 256 = {0, 16384} */
                else k0_spec_twiddle(zr[ib], zi[ib], tw[half - 1u + j], tr, ti);
                zr[ib] = zr[ia] - tr; zi[ib] = zi[ia] - ti;
                zr[ia] += tr; zi[ia] += ti;
            }
        }
    }
}

/* A wave's registers into the accumulators of capture s, slot `slot` (0 without ageing): one 64-bit atomic add and one atomic max per bin
 * that has something, and the count of the n level blocks they hold. */
__device__ __forceinline__ void k0_spec_flush(const K0SpecArgs &a, uint32_t s, uint32_t lane, uint64_t slot, const uint64_t (&acc)[8], const uint32_t (&top)[8],
                                              uint32_t n)
{
    uint64_t *sum = a.sum + slot * a.slot_stride + (uint64_t)s * WM_K0_SPEC_BINS;
    uint32_t *peak = a.peak + 2u * slot * a.slot_stride + (uint64_t)s * WM_K0_SPEC_BINS;
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++) {                          /* the lane holds j = 64 q + lane: bin (j + 256) mod 512 */
        const uint32_t b = 64u * (q ^ 4u) + lane;
        if (acc[q]) k0_add64(sum + b, acc[q]);
        if (top[q]) k0_max32(peak + b, top[q]);
    }
    if (lane == 0u) k0_add64(a.blocks + slot * a.slot_stride + s, (uint64_t)n);
}

/* v of the lane `step` away within its row of 16 lanes, for a value every lane of each aligned group of `step` lanes already shares (the
 * sum so far): steps 1 and 2 are quad permutations, 4 and 8 the mirrors of half a row and of a row.  The block emulator exchanges by xor. */
template <int STEP> __device__ __forceinline__ uint32_t k0_row_partner(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int ctrl = STEP == 1 ? 0xB1 : STEP == 2 ? 0x4E : STEP == 4 ? 0x141 : 0x140;
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xF, 0xF, false);
#else
    return __shfl_xor(v, STEP);
#endif
}
template <int STEP> __device__ __forceinline__ uint64_t k0_row_add(uint64_t v)
{
    return v + (((uint64_t)k0_row_partner<STEP>((uint32_t)(v >> 32)) << 32) | k0_row_partner<STEP>((uint32_t)v));
}
/* the sum of v over the lane's row of 16 lanes, in every lane of the row, clamped to 32 bits */
__device__ __forceinline__ uint32_t k0_row_sum_clamped(uint64_t v)
{
    v = k0_row_add<1>(v); v = k0_row_add<2>(v); v = k0_row_add<4>(v); v = k0_row_add<8>(v);
    return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
}

/* One block of WM_K0_SPEC_WAVES waves: blockIdx.x = four runs, blockIdx.y = capture.  lds: WM_K0_SPEC_WAVES x 2 x WM_K0_SPEC_PLANE dwords.
 * Lanes of a wave leave together or not at all. */
template <int FMT, bool DC, bool AGE = false, bool BANDS = false> __device__ __forceinline__ void k0_spectrum_block(const K0SpecArgs &a, int32_t *lds)
{
    constexpr uint32_t BPS = k0_bps(FMT), SPL = 16u / BPS, LOADS = (BPS << WM_K0_DC_LOG2) / (64u * 16u);
    static_assert(SPL * LOADS == 8u, "a lane loads 8 of a level block's 512 samples");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, s = blockIdx.y;
    uint32_t first = (blockIdx.x * (blockDim.x >> 6) + wave) * a.run;
    if (first >= a.n_blk) return;
    const uint32_t last = a.n_blk - first < a.run ? a.n_blk : first + a.run;
    uint32_t keep_from = first;                                  /* the first level block of the run that accumulates (BANDS: the ones in front of it are only written) */
    if constexpr (AGE) {                                         /* the level blocks of epochs below e_keep are a prefix of the push */
        const uint64_t k_keep = a.e_keep << a.age;
        if (k_keep > a.k_first) {
            const uint64_t skip = k_keep - a.k_first;
            if constexpr (BANDS) keep_from = skip >= last ? last : skip > first ? (uint32_t)skip : first;
            else {
                if (skip >= last) return;                        /* the same in every lane of the wave */
                first = skip > first ? (uint32_t)skip : first;
                keep_from = first;
            }
        }
    }
    int32_t *re = lds + wave * 2u * WM_K0_SPEC_PLANE, *im = re + WM_K0_SPEC_PLANE;
    const uint32_t *tab = a.shift_tab;

    /* what does not change over the run: the window of the lane's samples, the LDS slots of the layouts, the twiddles */
    /* the LDS slots of the layouts are a lane's base plus a constant per point: k0_spec_pad(n) = n + (n >> 3) splits so because every
     * constant part is a multiple of 8 */
    int32_t win[8];
    uint32_t tw0[7], tw1[7], tw2[7];
    const uint32_t rev = ((lane & 1u) << 5) | ((lane & 2u) << 3) | ((lane & 4u) << 1) | ((lane & 8u) >> 1) | ((lane & 16u) >> 3) | ((lane & 32u) >> 5);
    const uint32_t hi = lane >> 3, lo = lane & 7u;
    const uint32_t at_y = k0_spec_pad(lane * SPL);               /* sample (64 k + lane) SPL + r: + 72 SPL k + r */
    const uint32_t at_z = k0_spec_pad(rev);                      /* point 8 L + q is sample bitrev9(8 L + q) = 64 bitrev3(q) + bitrev6(L): + 72 bitrev3(q) */
    const uint32_t at_0 = k0_spec_pad(8u * lane);                /* point 8 L + q: + q */
    const uint32_t at_1 = k0_spec_pad(64u * hi) + lo;            /* point 64 hi + 8 q + lo: + 9 q */
    const uint32_t at_2 = k0_spec_pad(lane);                     /* point 64 q + L: + 72 q */
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++) {
        const uint32_t n = (64u * (q / SPL) + lane) * SPL + q % SPL;                 /* sample q of the lane's loads */
        win[q] = (16384 - (int32_t)(int16_t)(tab[2u * n] & 0xFFFFu) + 1) >> 1;
    }
    tw0[0] = tab[0]; tw0[1] = tab[0]; tw0[2] = tab[256]; tw0[3] = tab[0]; tw0[4] = tab[128]; tw0[5] = tab[256]; tw0[6] = tab[384];
#pragma unroll
    for (uint32_t t = 0; t < 3u; t++)
#pragma unroll
        for (uint32_t j = 0; j < (1u << t); j++) {                                   /* i = (j 8^P + p mod 8^P) (1024 >> stage) */
            tw1[(1u << t) - 1u + j] = tab[(8u * j + lo) * (64u >> t)];
            tw2[(1u << t) - 1u + j] = tab[(64u * j + lane) * (8u >> t)];
        }

    uint64_t acc[8];
    uint32_t top[8];
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++) { acc[q] = 0u; top[q] = 0u; }
    uint32_t since = keep_from;                                  /* AGE: the first level block the registers hold */

    for (uint32_t blk = first; blk < last; blk++) {
        if constexpr (AGE) {                                     /* an epoch edge inside the run: what the registers hold goes to its slot */
            const uint64_t e = (a.k_first + blk) >> a.age;
            if (blk > since && e != (a.k_first + since) >> a.age) {
                k0_spec_flush(a, s, lane, ((a.k_first + since) >> a.age) & 1u, acc, top, blk - since);
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) { acc[q] = 0u; top[q] = 0u; }
                since = blk;
            }
        }
        const uint8_t *p = a.raw + (uint64_t)s * a.raw_stride + ((uint64_t)blk << WM_K0_DC_LOG2) * BPS;
        K0U4 w[LOADS];
#pragma unroll
        for (uint32_t j = 0; j < LOADS; j++) w[j] = *(const K0U4 *)(p + 16u * (64u * j + lane));
        uint32_t dc = 0u;
        if constexpr (DC) dc = a.dc_tab[(uint64_t)s * a.dc_stride + blk];
        WM_K0_WAVE_SYNC();                                       /* the previous level block's last reads are done */
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
            const uint32_t in[4] = {w[q / SPL].x, w[q / SPL].y, w[q / SPL].z, w[q / SPL].w};
            uint32_t v = k0_sample_of<FMT>(in, q % SPL);
            if constexpr (DC) v = k0_sub_dc(v, dc);
            int32_t xi = (int32_t)(int16_t)(v & 0xFFFFu), xq = (int32_t)(int16_t)(v >> 16);
            if constexpr (FMT == WM_K0_CU8 || FMT == WM_K0_CS8) { xi *= 64; xq *= 64; }
            re[at_y + 72u * SPL * (q / SPL) + q % SPL] = (int32_t)k0_pair((xi * win[q] + 8192) >> 14, (xq * win[q] + 8192) >> 14);
        }
        WM_K0_WAVE_SYNC();
        int32_t zr[8], zi[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
            const uint32_t y = (uint32_t)re[at_z + 72u * (((q & 1u) << 2) | (q & 2u) | (q >> 2))];
            zr[q] = (int32_t)(int16_t)(y & 0xFFFFu); zi[q] = (int32_t)(int16_t)(y >> 16);
        }
        k0_spec_pass<true>(zr, zi, tw0);
        WM_K0_WAVE_SYNC();                                       /* every lane has read its y */
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) { re[at_0 + q] = zr[q]; im[at_0 + q] = zi[q]; }
        WM_K0_WAVE_SYNC();
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) { zr[q] = re[at_1 + 9u * q]; zi[q] = im[at_1 + 9u * q]; }
        k0_spec_pass<false>(zr, zi, tw1);
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) { re[at_1 + 9u * q] = zr[q]; im[at_1 + 9u * q] = zi[q]; }      /* the slots this lane has just read: no hazard */
        WM_K0_WAVE_SYNC();
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) { zr[q] = re[at_2 + 72u * q]; zi[q] = im[at_2 + 72u * q]; }
        k0_spec_pass<false>(zr, zi, tw2);
        uint32_t band = 0u;                                      /* BANDS: lane q of a row keeps the row's band of q */
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {                      /* |z| <= 2^23.5: the sum of the squares is below 2^48, pw below 2^32 */
            const uint64_t pw = ((uint64_t)((int64_t)zr[q] * zr[q]) + (uint64_t)((int64_t)zi[q] * zi[q])) >> 16;
            if constexpr (BANDS) {
                const uint32_t bp = k0_row_sum_clamped(pw);
                band = (lane & 15u) == q ? bp : band;
                if (AGE && blk < keep_from) continue;            /* a level block of an epoch the view no longer holds: written, not accumulated */
            }
            acc[q] += pw;
            top[q] = (uint32_t)pw > top[q] ? (uint32_t)pw : top[q];
        }
        if constexpr (BANDS) {                                   /* bins 64 (q ^ 4) + lane: band 4 (q ^ 4) + (lane >> 4), q = lane & 15 */
            if ((lane & 15u) < 8u) a.bands[(uint64_t)s * a.band_stride + 32u * (uint64_t)blk + 4u * ((lane & 15u) ^ 4u) + (lane >> 4)] = band;
        }
    }
    if constexpr (AGE) { if (!BANDS || last > since) k0_spec_flush(a, s, lane, ((a.k_first + since) >> a.age) & 1u, acc, top, last - since); }
    else k0_spec_flush(a, s, lane, 0u, acc, top, last - first);
}

#if defined(__HIPCC__)
template <int FMT, bool DC, bool AGE = false, bool BANDS = false> __global__ void __launch_bounds__(64 * WM_K0_SPEC_WAVES) k0_spectrum(K0SpecArgs a)
{
    __shared__ int32_t k0_spec_lds[WM_K0_SPEC_WAVES * 2u * WM_K0_SPEC_PLANE];
    k0_spectrum_block<FMT, DC, AGE, BANDS>(a, k0_spec_lds);
}
#endif

#endif
