/* wm_k2_clock_sys.h -- K2 clock recovery + time2 framer, SYSTOLIC form (round 6): a lane group's cascade on the four waves of a block.
 * Device code, included by wm_kernels.hip (one translation unit, see the overview there).
 *
 * What a lane computes, what it reads and what it leaves in memory is wm_k2_clock_lane.h's, shared with the one-wave form (wm_k2_clock.h)
 * to the word (start / end state records, checkpoints, chips, counts, slicer words, flags): the two forms are interchangeable launch by
 * launch, cfg.clock_waves picks one, and the host emulation runs them against each other.  What changes is WHO computes: lane l of a block
 * is four threads, one in each wave, and wave r carries role r of wm_k2_sys_blocks.h for all 64 lanes.
 *
 * Step s of a block, all four waves (k = s - b0, b0: the step at which the lane's segment was started):
 *     control   every thread learns its lane's control word of step s-1 (start a segment / lane finished)
 *     phase 1   role 0 reads the soft symbols of block k - 3 from the block's LDS rows, roles 1 and 2 the 32 values their predecessors
 *               left for blocks k - 4 / k - 5, role 3 the sample mask and slicer word of block k - 6
 *     barrier
 *     phase 2   roles 0 .. 2 compute and write their 32 values (role 2: the block's sample mask); the step's LOADER wave -- role 1 at even
 *               steps, role 3 at odd ones -- stages the soft symbols of block k - 2 (which it asked for two steps ago) into the rows and
 *               asks memory for block k; role 3 does the chips, slicer words, every record in memory and the lane's control word of
 *               block k - 6
 *     barrier
 * A lane's blocks are 32 samples; a ragged tail (< 32 samples at the end of a row) is role 3's alone, sample by sample, from the
 * lane state it has assembled anyway for the end record.  Lane state travels through LDS snapshots: after a block that ends a warm-up,
 * a checkpoint interval or the segment, roles 0 .. 2 leave their words for role 3, which meets them at its own step for that block.
 *
 * Lanes of a block need not march together (a re-run list mixes segments, lanes leave at checkpoints, walk chains): everything above is
 * per lane (b0, the segment's geometry, "has a block at this step"), only the two barriers and the loop's exit are the block's.
 *
 * Resources: 39.75 KB LDS (sizeof(ClkSysLds) = 40 704) and at most 128 VGPRs for 256 threads -- a block takes the place of ONE 512-thread
 * block of the demodulation kernel's first pass (35.2 KB, 64 VGPRs) plus part of the 22.6 KB four of those leave free on a CU.  (Round 6
 * measured the alternative with double-buffered hops, one barrier per step, 72 KB: 15 % faster alone and no faster than the one-wave form
 * beside a demodulation-shaped background, because its blocks wait for two neighbouring holes: tools/clkbench.hip.) */
#ifndef WM_K2_CLOCK_SYS_H
#define WM_K2_CLOCK_SYS_H

#include "wm_k2_sys_blocks.h"

/* word order of snap / start, nine words of a lane state: role 0's h1, h2 of section 0, dc_x, dc_y; role 1's h1, h2 of section 1;
 * role 2's h1, h2 of section 2, clk.  (Role 3 keeps the rest -- sr, pad -- itself.) */
enum { WM_SYSW_R0 = 0, WM_SYSW_R1 = 4, WM_SYSW_R2 = 6, WM_SYSW_N = 9 };

struct ClkSysLds {
    float x[64 * WM_CLK_XROW];               /* loader -> role 0: a block of soft symbols, one row per lane (transposed here when loaded cooperatively) */
    float hop[2][WM_SYS_HOP_WORDS];          /* role 0 -> role 1 -> role 2 */
    uint32_t chip[64 * WM_CLK_CROW];         /* role 3: chips waiting for a whole 32-byte group -- a ring of 16 per lane, chip n of a segment at [lane][n & 15]
                                                (rows of 17 words: the lanes' 4-byte accesses are bank-conflict free); a half that fills up leaves as it lies */
    uint32_t bits[8][64];                    /* role 3: slicer words waiting for a whole 32-byte group */
    uint32_t bitw[4][64];                    /* role 0 -> role 3: the slicer word of block b in slot b & 3 */
    uint32_t smask[64];                      /* role 2 -> role 3: the sample mask of the block role 2 has just done */
    uint32_t snap[2][WM_SYSW_N][64];         /* roles 0 .. 2 -> role 3: state words after a block (slot 1: the segment's last block) */
    uint32_t start[WM_SYSW_N][64];           /* role 3 -> roles 0 .. 2: state words a segment starts from */
    uint32_t ctl[2][64];                     /* role 3 -> all: control word of step s in slot s & 1 */
};
static_assert(sizeof(ClkSysLds) == 40704, "the header comment, DESIGN.md and the launch's place beside the demodulation kernel quote this size");

/* a lane's nine words (sr, pad: not among them) into / out of snap[slot] or start */
__device__ __forceinline__ void sys_words_put(uint32_t (*w)[64], const uint32_t ln, const WmClkState &st)
{
    w[WM_SYSW_R0][ln] = wm_f2u(st.h[0]); w[WM_SYSW_R0 + 1][ln] = wm_f2u(st.h[1]); w[WM_SYSW_R0 + 2][ln] = wm_f2u(st.dc_x); w[WM_SYSW_R0 + 3][ln] = wm_f2u(st.dc_y);
    w[WM_SYSW_R1][ln] = wm_f2u(st.h[2]); w[WM_SYSW_R1 + 1][ln] = wm_f2u(st.h[3]);
    w[WM_SYSW_R2][ln] = wm_f2u(st.h[4]); w[WM_SYSW_R2 + 1][ln] = wm_f2u(st.h[5]); w[WM_SYSW_R2 + 2][ln] = st.clk;
}
__device__ __forceinline__ void sys_words_get(const uint32_t (*w)[64], const uint32_t ln, WmClkState &st)
{
    st.h[0] = wm_u2f(w[WM_SYSW_R0][ln]); st.h[1] = wm_u2f(w[WM_SYSW_R0 + 1][ln]); st.dc_x = wm_u2f(w[WM_SYSW_R0 + 2][ln]); st.dc_y = wm_u2f(w[WM_SYSW_R0 + 3][ln]);
    st.h[2] = wm_u2f(w[WM_SYSW_R1][ln]); st.h[3] = wm_u2f(w[WM_SYSW_R1 + 1][ln]);
    st.h[4] = wm_u2f(w[WM_SYSW_R2][ln]); st.h[5] = wm_u2f(w[WM_SYSW_R2 + 1][ln]); st.clk = w[WM_SYSW_R2 + 2][ln];
}

enum { WM_SYS_NONE = 0, WM_SYS_START = 1, WM_SYS_NEXT = 2, WM_SYS_DONE = 3 };


/* -DWM_SYS_STAMPS (tools/sysbench.hip only): where a wave's cycles go -- control word, input reads + first barrier, work, second
 * barrier -- summed per wave into wm_sys_stamps[(block * 4 + role) * 4 ..] */
#if defined(WM_SYS_STAMPS)
__device__ unsigned long long *wm_sys_stamps;
#endif
#if defined(WM_SYS_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
#define WM_SYS_T0() unsigned long long st_t = __builtin_readcyclecounter(), st_acc[4] = {0, 0, 0, 0}
#define WM_SYS_MARK(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); st_acc[i] += t_ - st_t; st_t = t_; } while (0)
#define WM_SYS_DUMP() do { if (ln == 0 && wm_sys_stamps) for (int i_ = 0; i_ < 4; i_++) wm_sys_stamps[((size_t)blockIdx.x * 4 + role) * 4 + i_] = st_acc[i_]; } while (0)
#else
#define WM_SYS_T0() do {} while (0)
#define WM_SYS_MARK(i) do {} while (0)
#define WM_SYS_DUMP() do {} while (0)
#endif

/* after which blocks the lane state is recorded: the end of the warm-up (-> start record), interior checkpoints; slot 1: the last whole block */
__device__ __forceinline__ bool sys_snap0(const ClkGeo &G, uint32_t m, uint32_t nck)
{
    const uint32_t mn = m + 32u;
    if (m < G.mb) return mn == G.mb;
    return mn < G.me_full && (mn - G.mb) % (uint32_t)WM_CK_SAMPLES == 0u && (mn - G.mb) / (uint32_t)WM_CK_SAMPLES - 1u < nck;
}

/* The control word a lane meets at the top of a step.  A re-run lane's comes from role 3 through LDS (it leaves at checkpoints, walks
 * chains).  In the first pass a lane's life is known in advance -- started before step 0, finished when role 3 has done its last block,
 * b0 + nb + 5 -- so after step 0 nobody reads or writes control words (an LDS round trip at the top of every step of every wave: 280 of
 * 2 900 cycles per step, tools/sysbench.hip). */
template <int PASS>
__device__ __forceinline__ uint32_t sys_control(const ClkSysLds &lds, uint32_t step, uint32_t ln, bool valid, uint32_t b0, uint32_t nb)
{
    if (PASS == 0 && step != 0u) return valid && step - b0 == (nb ? nb + 6u : 1u) ? (uint32_t)WM_SYS_DONE : (uint32_t)WM_SYS_NONE;
    return lds.ctl[(step + 1u) & 1u][ln];
}

/* The LOADS.  Roles 1 and 3 take turns: role 1 at even steps, role 3 at odd ones.  At its step s = b0 + k a loader wave puts its
 * register set into the rows (the block it asked for at step s - 2: block k - 2 of the lane's walk, clamped into it) and asks for
 * block k; role 0 takes a block the step after it reached the rows, i.e. three steps after it was asked for.  So a wave has ONE set
 * in flight, asked for two steps before it is used, and its wait for the set is a wait for everything the wave has in flight --
 * which is what the compiler makes of any wait in these loops anyway (with both sets in one wave it drained the set asked for a step
 * ago as well: one block of lookahead, a step as long as a load's latency).  Unconditional for every lane: lanes without a segment
 * load row 0. */
__device__ __forceinline__ void sys_loader_step(const K2Args &a, const ClkLoad &ld, const bool coop, float *rows, wm_f4 (&gx)[8], const ClkGeo &G, const uint32_t k)
{
    clk_stage(ld, coop, rows, gx);
    clk_fetch(a, ld, coop, gx, G.m0 + 32u * min(k, G.nb ? G.nb - 1u : 0u));
}

/* PASS 0: the speculative first pass (every lane one segment), 1: a re-run list.  The lanes of chunk `group` (64 list entries / lane ids).
 * COOP (first pass of a batch of whole waves only): a wave is 64 consecutive captures of one (chain, segment) in lock step and loads
 * their soft symbols cooperatively -- a compile-time choice: as per-lane values the segment's geometry and the filter coefficients cost
 * every role some 50 vector instructions per step. */
template <bool DC, int PASS, bool COOP>
__device__ __forceinline__ void clock_sys_group(const K2Args &a, const uint32_t group, ClkSysLds &lds)
{
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t role = wm_uniform(threadIdx.x >> 6);
    const WmPush &g = a.g;
    constexpr bool rerun = PASS == 1;
    constexpr bool coop = COOP;
    static_assert(!(COOP && PASS == 1), "re-run lanes are not neighbours");

    /* ---- which segment is this lane's?  (every role works it out for itself) ---- */
    uint32_t lane = group * 64u + ln;
    bool valid = lane < k2_lane_count(a);
    if (valid && rerun) lane = a.list[lane];
    uint32_t ch = 0, stream = 0, seg = 0;
    if (valid) { lane_decode(g, 1, lane, ch, stream, seg); valid = (g.flags & (ch ? WM_F_S1 : WM_F_T1C1)) != 0u; }
    if (COOP) {
        /* the 64 lanes are 64 captures of ONE (chain, segment): said so, the segment's geometry, the kinds of its blocks, "has a block at
         * this step" and the filter coefficients live in scalar registers and the steps' branches are scalar branches */
        ch = wm_uniform(ch); seg = wm_uniform(seg); valid = wm_uniform((uint32_t)valid) != 0u;
    }
    const bool chains = rerun && a.bad != nullptr;
    const uint32_t *bad = clk_verdicts(a, ch, stream);    /* (chains only) */
    if (valid && chains && clk_chain_covered(a, bad, seg)) valid = false;
    const IirCoef c = iir_coef(ch);
    const uint32_t nck = a.nck;

    ClkGeo G = clk_geo(a, rerun, ch, stream, seg);
    uint32_t b0 = 0;
    bool active = false, finished = false;

    /* The top of a step, the same in every role: the lane's control word.  START / NEXT: the lane walks a segment from this step on -- the
     * roles that FOLLOW role 3 into the next segment of a chain make its geometry (role 3 made it when it decided), and each role does
     * what it does at a start (its start words).  DONE: the lane has finished.  Returns false when every lane of the block has: the same
     * answer in all four waves, the lanes' flags come from the control words. */
    auto step_control = [&](const uint32_t step, const bool follows, uint32_t &cw, auto at_start) WM_LAMBDA_INLINE -> bool {
        cw = sys_control<PASS>(lds, step, ln, valid, b0, G.nb);
        if (COOP) cw = wm_uniform(cw);
        const bool go = cw == WM_SYS_START || cw == WM_SYS_NEXT, stop = cw == WM_SYS_DONE;
        if (go) {
            if (follows && cw == WM_SYS_NEXT) { seg++; G = clk_geo(a, rerun, ch, stream, seg); }
            at_start();
            b0 = step;
        }
        /* (both flags are assigned on every path: two stores of `true` to one flag or the other, left to the optimiser inside a lambda,
         * become one store through a selected address, and then both flags live in scratch) */
        active = go || (active && !stop); finished = finished || stop;
        return __ballot(!finished) != 0ull;
    };
    wm_sys_barrier();                                     /* the previous chunk's last control words have been read */

    if (role == 0u) {
        /* ================= role 0: soft symbols -> [DC remover] -> slicer bits -> square -> section 0 ================= */
        float h1 = 0.0f, h2 = 0.0f, dcx = 0.0f, dcy = 0.0f;
        const float *xrow = lds.x + ln * WM_CLK_XROW;
        float *hop_out = lds.hop[0] + 4u * ln;
        wm_sys_barrier();                                   /* role 3 has set up every lane's first segment */
        WM_SYS_T0();
        for (uint32_t step = 0;; step++) {
            uint32_t cw;
            if (!step_control(step, true, cw, [&]() WM_LAMBDA_INLINE {
                    h1 = wm_u2f(lds.start[WM_SYSW_R0][ln]); h2 = wm_u2f(lds.start[WM_SYSW_R0 + 1][ln]);
                    dcx = wm_u2f(lds.start[WM_SYSW_R0 + 2][ln]); dcy = wm_u2f(lds.start[WM_SYSW_R0 + 3][ln]); })) break;
            WM_SYS_MARK(0);
            const uint32_t b = step - b0 - 3u;               /* (role 1 asks for block 0 in the step the start word arrives, and stages it two steps on) */
            const bool has = active && b < G.nb;
            wm_f4 x[8];
            if (has) {
#pragma unroll
                for (int q = 0; q < 8; q++) x[q] = *(const wm_f4 *)(xrow + 4 * q);       /* staged by a loader wave a step ago */
            }
            wm_sys_barrier();
            WM_SYS_MARK(1);
            if (has) {
                const uint32_t m = G.m0 + 32u * b;
                uint32_t bitw;
                if (clk_warm_short(G.mb, m)) sys_r0_block32<DC, true>(h1, h2, dcx, dcy, c, x, hop_out, bitw);
                else sys_r0_block32<DC, false>(h1, h2, dcx, dcy, c, x, hop_out, bitw);
                lds.bitw[b & 3u][ln] = bitw;
                const bool last = b + 1u == G.nb;
                if (last || sys_snap0(G, m, nck)) {
                    uint32_t (*sn)[64] = lds.snap[last ? 1 : 0];
                    sn[WM_SYSW_R0][ln] = wm_f2u(h1); sn[WM_SYSW_R0 + 1][ln] = wm_f2u(h2); sn[WM_SYSW_R0 + 2][ln] = wm_f2u(dcx); sn[WM_SYSW_R0 + 3][ln] = wm_f2u(dcy);
                }
            }
            WM_SYS_MARK(2);
            wm_sys_barrier();
            WM_SYS_MARK(3);
        }
        WM_SYS_DUMP();
    } else if (role == 1u) {
        /* ================= role 1: section 1 + the loads of the even steps ================= */
        float h1 = 0.0f, h2 = 0.0f;
        const float *hop_in = lds.hop[0] + 4u * ln;
        float *hop_out = lds.hop[1] + 4u * ln;
        wm_f4 gx[8];
        ClkLoad ld = clk_load_init(a, G, coop, ln);
        wm_sys_barrier();                                   /* role 3 has set up every lane's first segment */
        clk_fetch(a, ld, coop, gx, 0u);                     /* the set starts out defined */
        WM_SYS_T0();
        for (uint32_t step = 0;; step++) {
            /* the input block is asked for before the control word is looked at (one LDS round trip, not two): a lane that is told to
             * start or to stop has no block of its own in this step */
            const uint32_t b = step - b0 - 4u;
            const bool has0 = active && b < G.nb;
            wm_f4 in[8];
            if (has0) sys_hop_read(hop_in, in);
            uint32_t cw;
            if (!step_control(step, true, cw, [&]() WM_LAMBDA_INLINE {
                    h1 = wm_u2f(lds.start[WM_SYSW_R1][ln]); h2 = wm_u2f(lds.start[WM_SYSW_R1 + 1][ln]);
                    clk_load_segment(ld, a, G, ln); })) break;
            WM_SYS_MARK(0);
            const bool has = has0 && cw == WM_SYS_NONE;
            wm_sys_barrier();
            WM_SYS_MARK(1);
            if ((step & 1u) == 0u) sys_loader_step(a, ld, coop, lds.x, gx, G, step - b0);
            if (has) {
                const uint32_t m = G.m0 + 32u * b;
                sys_r1_block32(h1, h2, c, in, hop_out);
                const bool last = b + 1u == G.nb;
                if (last || sys_snap0(G, m, nck)) {
                    uint32_t (*sn)[64] = lds.snap[last ? 1 : 0];
                    sn[WM_SYSW_R1][ln] = wm_f2u(h1); sn[WM_SYSW_R1 + 1][ln] = wm_f2u(h2);
                }
            }
            WM_SYS_MARK(2);
            wm_sys_barrier();
            WM_SYS_MARK(3);
        }
        WM_SYS_DUMP();
    } else if (role == 2u) {
        /* ================= role 2: section 2, level, clock lock ================= */
        float h1 = 0.0f, h2 = 0.0f;
        uint32_t clk = 0;
        const float *hop_in = lds.hop[1] + 4u * ln;
        wm_sys_barrier();                                   /* role 3 has set up every lane's first segment */
        WM_SYS_T0();
        for (uint32_t step = 0;; step++) {
            const uint32_t b = step - b0 - 5u;
            const bool has0 = active && b < G.nb;
            wm_f4 in[8];
            if (has0) sys_hop_read(hop_in, in);
            uint32_t cw;
            if (!step_control(step, true, cw, [&]() WM_LAMBDA_INLINE {
                    h1 = wm_u2f(lds.start[WM_SYSW_R2][ln]); h2 = wm_u2f(lds.start[WM_SYSW_R2 + 1][ln]); clk = lds.start[WM_SYSW_R2 + 2][ln]; })) break;
            WM_SYS_MARK(0);
            const bool has = has0 && cw == WM_SYS_NONE;
            wm_sys_barrier();
            WM_SYS_MARK(1);
            if (has) {
                const uint32_t m = G.m0 + 32u * b;
                uint32_t smask;
                if (clk_warm_short(G.mb, m)) sys_r2_block32<true>(h1, h2, clk, c, in, smask); else sys_r2_block32<false>(h1, h2, clk, c, in, smask);
                lds.smask[ln] = smask;
                const bool last = b + 1u == G.nb;
                if (last || sys_snap0(G, m, nck)) {
                    uint32_t (*sn)[64] = lds.snap[last ? 1 : 0];
                    sn[WM_SYSW_R2][ln] = wm_f2u(h1); sn[WM_SYSW_R2 + 1][ln] = wm_f2u(h2); sn[WM_SYSW_R2 + 2][ln] = clk;
                }
            }
            WM_SYS_MARK(2);
            wm_sys_barrier();
            WM_SYS_MARK(3);
        }
        WM_SYS_DUMP();
    } else {
        /* ================= role 3: time2 chips, slicer words, every record in memory, the loads of the odd steps ================= */
        /* of the lane state only the time2 shift register (and the padding words, as loaded) lives here between records: the rest is
         * gathered from the other roles' snapshots where a record is written -- a whole WmClkState across the loop is 12 of 128 VGPRs */
        uint32_t sr = 0, pad0 = 0, pad1 = 0;
        const ClkSync y = clk_sync(a, ch);
        uint32_t *my_chip = lds.chip + ln * WM_CLK_CROW;
        auto ring = [&](uint32_t n) WM_LAMBDA_INLINE -> uint32_t & { return my_chip[n & 15u]; };
        uint32_t *out = a.chips, *ck = a.ckpt, *bw = a.bits;
        uint32_t n_fl = 0, pend = 0, saw_sync = 0;
        wm_f4 gx[8];
        ClkLoad ld = clk_load_init(a, G, coop, ln);

        auto gather = [&](const uint32_t (*w)[64]) WM_LAMBDA_INLINE -> WmClkState {      /* the other roles' words (a snapshot, the start words) + my own */
            WmClkState t;
            sys_words_get(w, ln, t);
            t.sr = sr; t.pad[0] = pad0; t.pad[1] = pad1;
            return t;
        };
        /* a segment is made ready a step before the other roles learn of it: geometry, output pointers, the start record of a walk
         * without warm-up, the start words */
        auto launch_segment = [&](const WmClkState &st) WM_LAMBDA_INLINE {
            G = clk_geo(a, rerun, ch, stream, seg);
            out = a.chips + G.sidx * g.cap[1];
            ck = a.ckpt + G.sidx * (uint64_t)nck * 16u;
            bw = a.bits + G.row * (g.Mcap / 32);
            n_fl = 0; pend = 0; saw_sync = 0;
            if (G.m0 == G.mb) ((WmClkState *)a.st_start)[G.sidx] = st;
            sys_words_put(lds.start, ln, st);
            sr = st.sr; pad0 = st.pad[0]; pad1 = st.pad[1];
            clk_load_segment(ld, a, G, ln);
        };
        /* Chips leave in whole, 32-byte aligned groups of 8; n_fl is a multiple of 8: the ring's half (n_fl & 8) is the group and leaves
         * as it lies.  (Role 3 has no arithmetic to hide the read behind and no need to: it is the wave with time to spare.) */
        auto flush8 = [&]() WM_LAMBDA_INLINE {
            const uint32_t *h = my_chip + (n_fl & 8u);
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = h[i];
            *(uint4 *)(out + n_fl) = make_uint4(w[0], w[1], w[2], w[3]);
            *(uint4 *)(out + n_fl + 4) = make_uint4(w[4], w[5], w[6], w[7]);
            n_fl += 8u; pend = pend > 8u ? pend - 8u : 0u;
        };
        /* The end of a lane's segment and what comes after it, in ONE place of a step (three places reach it: the last whole block, a
         * checkpoint a re-run reproduces, a segment without a whole block): clk_segment_end, then clk_chain_next: nothing more, or (a
         * re-run lane walking its chain) the next segment from the exact end state.
         * how: 1 = the segment ran to its end, `fin` is the state after its last whole block; 2 = it left at a checkpoint. */
        auto finish_lane = [&](uint32_t how, WmClkState &fin) WM_LAMBDA_INLINE -> uint32_t {
            if (how == 1u) {
                const uint32_t n_out = n_fl + pend;
                if (pend) flush8();                          /* last group; slots beyond n_out are never read */
                clk_segment_end<DC>(a, G, c, y, fin, out, bw, n_out, saw_sync, g.cap[1], G.sidx);
            }
            if (!chains || !clk_chain_next(a, bad, how == 2u, seg, G.sidx, fin)) return WM_SYS_DONE;
            seg++;
            launch_segment(fin);
            return WM_SYS_NEXT;
        };

        /* ---- before step 0: the lane's first segment ---- */
        uint32_t cmd = WM_SYS_DONE;
        if (valid) {
            launch_segment(clk_start_state(a, G, rerun, ch, seg));
            cmd = WM_SYS_START;
        }
        lds.ctl[1][ln] = cmd;
        wm_sys_barrier();

        clk_fetch(a, ld, coop, gx, 0u);                     /* the set starts out defined */
        WM_SYS_T0();
        for (uint32_t step = 0;; step++) {
            const uint32_t bc = step - b0 - 6u;              /* the block whose chips are due */
            const bool has0 = active && bc < G.nb;
            uint32_t smask = 0, bitw = 0;                    /* what roles 2 and 0 left for that block: nothing in the block waits for LDS */
            if (has0) { smask = lds.smask[ln]; bitw = lds.bitw[bc & 3u][ln]; }
            cmd = WM_SYS_NONE;
            uint32_t how = 0;                                /* the lane's segment ends in this step: 1 at its end, 2 at a checkpoint */
            uint32_t cw;                                     /* (fewer than 32 samples: all of the segment is the tail, from the start state) */
            if (!step_control(step, false, cw, [&]() WM_LAMBDA_INLINE { if (G.nb == 0u) how = 1u; })) break;
            WM_SYS_MARK(0);
            const bool has = has0 && cw == WM_SYS_NONE;
            wm_sys_barrier();
            WM_SYS_MARK(1);
            if ((step & 1u) == 1u) sys_loader_step(a, ld, coop, lds.x, gx, G, step - b0);
            if (has) {
                const uint32_t m = G.m0 + 32u * bc;
                const bool last = bc + 1u == G.nb;
                if (m < G.mb) {
                    /* ---- warm-up block ---- */
                    if (!clk_warm_short(G.mb, m)) clk_warm_chips(sr, smask, bitw, y, G.mb - m);
                    if (m + 32u == G.mb) {                                         /* state the segment proper starts from */
                        /* fewer than 32 samples after the warm-up: this block is also the last one (roles 0 .. 2 posted it in slot 1),
                         * and all of the segment is the ragged tail */
                        ((WmClkState *)a.st_start)[G.sidx] = gather(lds.snap[last ? 1 : 0]);
                        if (last) how = 1u;
                    }
                } else {
                    /* ---- block of the segment proper: chips into the staging ring (a block's slots are at most 7 + 7 ahead of n_fl: never a
                     * waiting chip), whole groups to memory ---- */
                    const uint32_t cnt = clk_block_chips(sr, saw_sync, smask, bitw, y, m - G.mb, [&](int i) WM_LAMBDA_INLINE -> uint32_t & { return ring(n_fl + pend + i); });
                    pend += y.t2a ? cnt : 0u;
                    if (pend >= 8u) flush8();
                    if (!clk_bits_put(bw, &lds.bits[0][ln], 64u, m >> 5, bitw) && last) clk_bits_rest(bw, &lds.bits[0][ln], 64u, (m >> 5) + 1u);
                    if (last) how = 1u;
                    else if (sys_snap0(G, m, nck) &&
                             clk_checkpoint(a, rerun, gather(lds.snap[0]), ck, (m + 32u - G.mb) / (uint32_t)WM_CK_SAMPLES - 1u, nck, G.sidx, out, n_fl, pend, saw_sync,
                                            [&](uint32_t i) WM_LAMBDA_INLINE { return ring(n_fl + i); })) how = 2u;
                }
            }
            if (how) {
                WmClkState fin = gather(G.nb == 0u ? lds.start : lds.snap[1]);      /* (how == 2: replaced by the recorded end state) */
                cmd = finish_lane(how, fin);
                active = false;
            }
            if (PASS != 0) lds.ctl[step & 1u][ln] = cmd;
            WM_SYS_MARK(2);
            wm_sys_barrier();
            WM_SYS_MARK(3);
        }
        WM_SYS_DUMP();
    }
}

#if defined(__HIPCC__)
/* The block's LDS is DYNAMIC (sizeof(ClkSysLds) at the launch): with a static array of that size the compiler works out that at most three blocks
 * fit a CU, drops the request for four waves per SIMD as unachievable and allocates 200+ VGPRs -- and a wave that wide needs the
 * registers of TWO demodulation blocks to leave before it can start.  What matters is not how many clock blocks fit a CU (one,
 * rarely two) but that one fits wherever a demodulation block has just left: 128 VGPRs. */
extern __shared__ __attribute__((aligned(16))) unsigned char wm_sys_lds[];

template <bool DC, bool COOP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k2_clock_sys(K2Args a)                 /* first pass: one block per 64 lanes; COOP: a.g.S % 64 == 0 */
{
    wm_framer_prio();
    clock_sys_group<DC, 0, COOP>(a, blockIdx.x, *(ClkSysLds *)wm_sys_lds);
}

template <bool DC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k2_clock_sys_list(K2Args a)            /* re-run list: a fixed grid whose blocks walk the list, 64 entries at a time */
{
    wm_framer_prio();
    const uint32_t n = k2_lane_count(a);
    for (uint32_t b = blockIdx.x; (uint64_t)b * 64u < n; b += gridDim.x) clock_sys_group<DC, 1, false>(a, b, *(ClkSysLds *)wm_sys_lds);
}

#endif /* __HIPCC__ */

#endif /* WM_K2_CLOCK_SYS_H */
