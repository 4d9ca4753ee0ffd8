/* wm_k2_clock.h -- K2 clock recovery + time2 framer lanes, ONE-WAVE form: a lane is one thread that carries the whole cascade.
 * Device code, included by wm_kernels.hip (one translation unit, see the overview there).  What a lane is -- its records, its chips,
 * its rules -- is wm_k2_clock_lane.h's, shared with the systolic form (wm_k2_clock_sys.h); this file owns the cascade of a 32-sample
 * block in one thread, the two register sets of soft symbols in flight and the chips' compacted staging row. */
#ifndef WM_K2_CLOCK_H
#define WM_K2_CLOCK_H

#include "wm_k2_clock_lane.h"

/* 32 samples through [DC remover] -> x^2 -> 3 biquads -> clock level, SOFTWARE-PIPELINED across the
 * filter sections: at tick t section k works on sample t - k, so the three (four with -o) recurrences
 * of a tick are independent instruction streams; a lone wave issues a dependent VALU operation only
 * every ~8.5 cycles on gfx950, and the straight per-sample order is one 36-deep dependent chain.
 * The compiler's scheduler would undo the interleaving (it sinks each section's recurrence into one
 * serial run over the block), so the levels of a tick are fenced with sched_barrier.  The pipeline
 * drains at the end of the block: the lane state at block boundaries is the plain sequential
 * state.  Every value is produced by exactly the operations of iir.h:57-74 / rtl_wmbus.c:497-515.
 *
 * Bits: the slicer output (soft >= 0, rtl_wmbus.c:1059) is the inverted sign bit -- a soft symbol
 * is never -0 (the FIR accumulates from +0, and +0 + -0 = +0; the DC remover's x - x_old is never
 * -0 either) -- shifted into a word with one v_alignbit; clock levels via WM_LEVEL_CARRY. */
/* WARM (round 5): a warm-up block whose chips nobody looks at (it ends more than WM_CLK_SR_WINDOW samples before the segment) --
 * the recurrences of all three sections run as ever, but what only FEEDS THE OUTPUT is left out: the last section's feed-forward
 * half and the level (6 instructions), the slicer bit (1): 20 instead of 27 per sample.  s.clk is not touched; the full blocks
 * behind it (at least WM_CLK_SR_WINDOW / 32 + 1 of them) set it. */
template <bool DC, bool WARM = false>
__device__ __forceinline__ void clk_block32(WmClkState &s, const IirCoef &c, const float *xrow, uint32_t &bitw, uint32_t &smask)
{
    /* xrow: this lane's 32 soft symbols in LDS; four are fetched every fourth tick, so the block in
     * flight and the one after it can stay in registers (two blocks of loads outstanding per lane) */
    float4 xq = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int P = DC ? 1 : 0;                          /* pipeline depth before the first biquad */
    float h1[3] = {s.h[0], s.h[2], s.h[4]}, h2[3] = {s.h[1], s.h[3], s.h[5]};
    float dcx = s.dc_x, dcy = s.dc_y;
    float in[3] = {0.0f, 0.0f, 0.0f};                      /* input of section k at the coming tick */
    float soft = 0.0f;                                     /* DC stage output waiting for section 0 */
    uint32_t sgn = 0, low = 0;                             /* MSB-first: sample n ends up in bit 31 - n */
    const float al = 0.999f, kk = wm_div(wm_add(1.0f, al), 2.0f);
#pragma unroll
    for (int t = 0; t < 32 + P + 2; t++) {
        float m1[3], m2[3], p1[3], p2[3], tt[3], h0[3], u[3], o[3];
        float d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
        if (t < 32 && (t & 3) == 0) xq = *(const float4 *)(xrow + t);
        const float xt = (t & 3) == 0 ? xq.x : (t & 3) == 1 ? xq.y : (t & 3) == 2 ? xq.z : xq.w;   /* sample t (t < 32) */
        /* level 1: every product that only needs last tick's state */
        if (DC && t < 32) { d1 = wm_sub(xt, dcx); d2 = wm_mul(al, dcy); }
        {   /* section 0's input: the (DC-filtered) soft symbol, squared */
            const int n0 = t - P;
            if (n0 >= 0 && n0 < 32) {
                const float sf = DC ? soft : xt;
                if (!WARM) sgn = __builtin_amdgcn_alignbit(sgn, wm_f2u(sf), 31);      /* (sgn << 1) | signbit */
                in[0] = wm_mul(sf, sf);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int n = t - P - k;
            if (n >= 0 && n < 32) {
                m1[k] = wm_mul(c.a1[k], h1[k]); m2[k] = wm_mul(c.a2[k], h2[k]);
                if (!(WARM && k == 2)) { p1[k] = wm_mul(c.b1[k], h1[k]); p2[k] = wm_mul(c.b2[k], h2[k]); }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        /* level 2 */
        if (DC && t < 32) d3 = wm_mul(kk, d1);
#pragma unroll
        for (int k = 0; k < 3; k++) { const int n = t - P - k; if (n >= 0 && n < 32) tt[k] = wm_add(m1[k], m2[k]); }
        __builtin_amdgcn_sched_barrier(0);
        /* level 3 */
        if (DC && t < 32) { const float y = wm_add(d3, d2); dcx = xt; dcy = y; soft = y; }
#pragma unroll
        for (int k = 0; k < 3; k++) { const int n = t - P - k; if (n >= 0 && n < 32) h0[k] = wm_sub(in[k], tt[k]); }
        __builtin_amdgcn_sched_barrier(0);
        /* level 4, 5 */
#pragma unroll
        for (int k = 0; k < 3; k++) { const int n = t - P - k; if (n >= 0 && n < 32 && !(WARM && k == 2)) u[k] = wm_add(h0[k], p1[k]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 3; k++) { const int n = t - P - k; if (n >= 0 && n < 32 && !(WARM && k == 2)) o[k] = wm_add(u[k], p2[k]); }
        /* hand over: section k's output is section k+1's input at the next tick */
#pragma unroll
        for (int k = 2; k >= 0; k--) {
            const int n = t - P - k;
            if (n >= 0 && n < 32) {
                h2[k] = h1[k]; h1[k] = h0[k];
                if (k < 2) in[k + 1] = o[k];
                else if (!WARM) low = wm_shift_in_level_low(low, wm_f2u(o[2]));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    s.h[0] = h1[0]; s.h[1] = h2[0]; s.h[2] = h1[1]; s.h[3] = h2[1]; s.h[4] = h1[2]; s.h[5] = h2[2];
    s.dc_x = dcx; s.dc_y = dcy;
    if (WARM) { bitw = 0u; smask = 0u; return; }
    bitw = ~__builtin_bitreverse32(sgn);
    smask = clk_lock_mask(low, s.clk);
}

template <int W> struct ClkLds {         /* per block: W independent waves */
    float x[W][64 * WM_CLK_XROW];
    uint32_t chip[W][64 * WM_CLK_CROW];
    uint32_t bits[W][64 * WM_CLK_BROW];
};

/* WM_CLK_WPB independent waves per block (no block-wide barrier anywhere): a block's waves land on
 * the CU's four SIMDs, so the framer loads every SIMD of the CUs it is on equally.  A lone
 * long-running wave on ONE SIMD slows every 4-wave K1 block of that CU down to the pace of the K1
 * wave that shares the SIMD with it (measured: two clock launches in flight, one wave per CU, cost
 * K1 60 %). */
/* PASS: 0 = the speculative first pass only (a.list == nullptr), 1 = a re-run list only, 2 = either (host emulation): each kind of launch has its own
 * kernel, so the first pass carries neither the list walk nor the checkpoint comparison (with both in one kernel behind
 * a grid-stride loop the first pass needed 254 VGPRs + 16 AGPRs and ran at one wave per SIMD, round 2). */
/* One segment of one (chain, capture): returns 0 when the lane ran to the segment's end (`fin` = its end state, also written to
 * st_final), 1 when a re-run left early at a checkpoint it reproduced (the end state in st_final was exact already), 2 when
 * there was nothing to do.  `from` (with have_from): the exact state a re-run starts from when the caller has it at hand (else:
 * clk_start_state).  By value, not by pointer: a pointer that may name the caller's `fin` kept both in scratch. */
template <bool DC, int W, int PASS>
__device__ __forceinline__ int clock_segment(const K2Args &a, ClkLds<W> &lds, const uint32_t wv, const uint32_t ln, const bool rerun,
                                             const uint32_t ch, const uint32_t stream, const uint32_t seg, const bool have_from, const WmClkState &from, WmClkState &fin)
{
    float *s_x = lds.x[wv];
    const WmPush &g = a.g;
    const bool coop = !rerun && (g.S % 64u) == 0u;         /* wave = 64 consecutive streams, lock step */

    /* S1 lanes may span two segments (WmPush.s1_span): the odd segment rides with its even predecessor.  The lane then
     * owns both segments' chip regions, checkpoint slots and hand-off records (they are adjacent): chips and count go to
     * the even one (the odd one's count is 0), the end state to the odd one's record, and the pair (final[even],
     * start[odd]) is set to one constant so that the verifier, which knows nothing of this, sees a certified hand-off. */
    const uint32_t span = (ch == 1u && g.s1_span == 2u) ? 2u : 1u;
    if (seg % span) return 2;
    const ClkGeo G = clk_geo(a, rerun, ch, stream, seg, span);
    const uint32_t covered = (G.me - G.mb + g.seg_len[1] - 1u) / g.seg_len[1];      /* segments this lane really covers: 1 or 2 */
    const uint32_t cap_t2 = covered * g.cap[1];
    const uint32_t nck = covered == 2u ? 2u * a.nck : a.nck;                          /* checkpoint slots (one interior point of a pair has none) */
    const uint64_t sidxF = G.sidx + covered - 1u;                                     /* where the end state goes */
    WmClkState *stS = (WmClkState *)a.st_start, *stF = (WmClkState *)a.st_final;

    WmClkState s;
    if (have_from) s = from; else s = clk_start_state(a, G, rerun, ch, seg);
    uint32_t m = G.m0;
    const IirCoef c = iir_coef(ch);
    const ClkSync y = clk_sync(a, ch);
    uint32_t *out = a.chips + G.sidx * g.cap[1];          /* region pitch (cap_t2 may be two regions) */
    uint32_t *bw = a.bits + G.row * (g.Mcap / 32);
    uint32_t saw_sync = 0;

    /* Two blocks of loads are kept in flight per lane (register sets A and B, used alternately):
     * with one, the kernel ran at the latency of a single 10 KB request per wave (2.8 TB/s). */
    wm_f4 gxA[8], gxB[8];
    const ClkLoad ld = clk_load_init(a, G, coop, ln);
    const float *xrow = s_x + ln * WM_CLK_XROW;
    auto next_x = [&](wm_f4 (&gx)[8]) WM_LAMBDA_INLINE { clk_stage(ld, coop, s_x, gx); clk_fetch(a, ld, coop, gx, m + 64u); };

    /* ---- phase 1: warm-up blocks [m, mb): soft symbols only; no store is issued in this loop, so
     * waiting for a block in flight never waits for anything else (gfx950's vmcnt counts loads
     * and stores in one in-order queue) --------------------------------------------------------- */
    auto warm_block = [&](wm_f4 (&gx)[8]) WM_LAMBDA_INLINE {
        next_x(gx);
        uint32_t bitw, smask;
        if (clk_warm_short(G.mb, m)) clk_block32<DC, true>(s, c, xrow, bitw, smask);
        else clk_block32<DC>(s, c, xrow, bitw, smask);
        clk_warm_chips(s.sr, smask, bitw, y, G.mb - m);
        m += 32;
    };
    if (m < G.me_full) { clk_fetch(a, ld, coop, gxA, m); clk_fetch(a, ld, coop, gxB, m + 32u); }
    while (m < G.mb) {
        warm_block(gxA);
        if (m < G.mb) warm_block(gxB);
        else {                                               /* keep "A = next block" for phase 2 */
#pragma unroll
            for (int i = 0; i < 8; i++) { const wm_f4 t = gxA[i]; gxA[i] = gxB[i]; gxB[i] = t; }
        }
    }
    stS[G.sidx] = s;                                     /* state the main loop starts from */
    /* ---- phase 2: blocks of the segment proper.  Exactly three stores per block (slicer word and
     * two 16-byte chip stores; a block holds at most 8 chips, and slots beyond the block's chips are
     * overwritten by the next block), so the compiler can wait for a prefetched block with a counted
     * vmcnt instead of draining the stores. */
    /* chips leave in whole, 32-byte aligned groups of 8: the first eight of the staging row, the rest moves down */
    uint32_t *my_chip = lds.chip[wv] + ln * WM_CLK_CROW, *my_bits = lds.bits[wv] + ln * WM_CLK_BROW;
    uint32_t pend = 0, n_fl = 0;
    auto flush8 = [&]() WM_LAMBDA_INLINE {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = my_chip[i];
        *(uint4 *)(out + n_fl) = make_uint4(w[0], w[1], w[2], w[3]);
        *(uint4 *)(out + n_fl + 4) = make_uint4(w[4], w[5], w[6], w[7]);
#pragma unroll
        for (int i = 0; i < 8; i++) { const uint32_t v = my_chip[8 + i]; if (8u + i < pend) my_chip[i] = v; }
        n_fl += 8u; pend = pend > 8u ? pend - 8u : 0u;
    };
    auto main_block = [&](wm_f4 (&gx)[8]) WM_LAMBDA_INLINE {
        next_x(gx);
        uint32_t bitw, smask;
        clk_block32<DC>(s, c, xrow, bitw, smask);
        const uint32_t cnt = clk_block_chips(s.sr, saw_sync, smask, bitw, y, m - G.mb, [&](int i) WM_LAMBDA_INLINE -> uint32_t & { return my_chip[pend + i]; });
        pend += y.t2a ? cnt : 0u;
        clk_bits_put(bw, my_bits, 1u, m >> 5, bitw);
        if (pend >= 8u) flush8();
        m += 32;
    };
    uint32_t *ck = a.ckpt + G.sidx * (uint64_t)a.nck * 16u;
    for (uint32_t j = 0; m < G.me_full; j++) {
        const uint32_t stop = min(G.me_full, m + (uint32_t)WM_CK_SAMPLES);   /* an even number of blocks, or the end */
        while (m < stop) {
            main_block(gxA);
            if (m < stop) main_block(gxB);
        }
        if (m < G.me_full && j < nck &&
            clk_checkpoint(a, rerun, s, ck, j, nck, G.sidx, out, n_fl, pend, saw_sync, [&](uint32_t i) WM_LAMBDA_INLINE { return my_chip[i]; })) return 1;
    }
    clk_bits_rest(bw, my_bits, 1u, m >> 5);
    const uint32_t n_out = n_fl + pend;
    if (pend) flush8();                                  /* last group; slots beyond n_out are never read */
    clk_segment_end<DC>(a, G, c, y, s, out, bw, n_out, saw_sync, cap_t2, sidxF);
    if (covered == 2u) { const WmClkState none = {}; stF[G.sidx] = none; stS[G.sidx + 1u] = none; a.counts[G.sidx + 1u] = 0u; }
    fin = s;
    return 0;
}

/* The lanes of one launch.  First pass: lane = (chain, segment, capture), every lane one segment.  Re-run list: a listed lane does its
 * segment, or walks its CHAIN (wm_k2_clock_lane.h: clk_chain_next), one segment after the other from the exact end state of the one before. */
template <bool DC, int W, int PASS = 2>
__device__ __forceinline__ void clock_lanes(const K2Args &a, const uint32_t block, ClkLds<W> &lds)
{
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (wv >= (uint32_t)W) return;
    uint32_t lane = (block * W + wv) * 64 + ln;
    const bool rerun = PASS == 2 ? a.list != nullptr : PASS == 1;
    const WmPush &g = a.g;
    if (lane >= k2_lane_count(a)) return;
    if (rerun) lane = a.list[lane];
    uint32_t ch, stream, seg;
    lane_decode(g, 1, lane, ch, stream, seg);
    if (!(g.flags & (ch ? WM_F_S1 : WM_F_T1C1))) return;
    WmClkState fin, from{};
    const bool chains = rerun && a.bad != nullptr && !(ch == 1u && g.s1_span == 2u);
    if (!chains) { clock_segment<DC, W, PASS>(a, lds, wv, ln, rerun, ch, stream, seg, false, from, fin); return; }
    const uint32_t *bad = clk_verdicts(a, ch, stream);
    if (clk_chain_covered(a, bad, seg)) return;
    const uint64_t sidx0 = ((uint64_t)ch * g.S + stream) * g.nseg_cap[1];
    bool have_from = false;
    for (;;) {
        const int how = clock_segment<DC, W, PASS>(a, lds, wv, ln, true, ch, stream, seg, have_from, from, fin);
        if (how == 2 || !clk_chain_next(a, bad, how == 1, seg, sidx0 + seg, fin)) return;
        seg++;
        from = fin; have_from = true;
    }
}

template <bool DC>
__global__ __launch_bounds__(64 * WM_CLK_WPB) void k2_clock(K2Args a)                 /* first pass: one block per 64 * WM_CLK_WPB lanes */
{
    wm_framer_prio();
    __shared__ __attribute__((aligned(16))) ClkLds<WM_CLK_WPB> lds;
    clock_lanes<DC, WM_CLK_WPB, 0>(a, blockIdx.x, lds);
}

template <bool DC>
__global__ __launch_bounds__(64 * WM_CLK_WPB) void k2_clock_list(K2Args a)            /* re-run list: a fixed grid whose blocks walk the list */
{
    wm_framer_prio();
    __shared__ __attribute__((aligned(16))) ClkLds<WM_CLK_WPB> lds;
    const uint32_t n = k2_lane_count(a);
    for (uint32_t b = blockIdx.x; (uint64_t)b * (64u * WM_CLK_WPB) < n; b += gridDim.x) clock_lanes<DC, WM_CLK_WPB, 1>(a, b, lds);
}

#endif /* WM_K2_CLOCK_H */
