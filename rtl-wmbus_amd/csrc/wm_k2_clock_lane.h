/* wm_k2_clock_lane.h -- K2 clock recovery + time2 framer: what a LANE is, whoever does its arithmetic.
 * Device code, included by wm_k2_clock.h (one wave per lane group) and wm_k2_sys_blocks.h (four roles on four waves).
 *
 * The two forms leave memory identical to the word -- start and end records, checkpoints, chips, counts, slicer words, flags -- and
 * everything that decides those words is here, once: a filter section's step, the lock pattern, a segment's geometry and start state,
 * the soft symbols' way from memory into the LDS rows, the chip loops of a block, the slicer words' groups, the checkpoint rule, the
 * segment's epilogue and the chain walk's decision.  A form owns its schedule (who computes which block when) and its chip staging.
 *
 * Every helper is inlined and takes register sets as wm_f4 (&)[8]: a lane's register sets taken by reference by a lambda or helper that
 * is left out of line (or inlined late) live in scratch memory -- in the re-run kernel that cost every 32-sample block sixteen scratch
 * accesses AND the prefetch (a block of loads had to arrive before it could be stored away; round 5, read off the ISA). */
#ifndef WM_K2_CLOCK_LANE_H
#define WM_K2_CLOCK_LANE_H

#if defined(__clang__)
#define WM_LAMBDA_INLINE __attribute__((always_inline))
#else
#define WM_LAMBDA_INLINE
#endif

/* the lane's register sets are NATIVE vectors: a float4 (HIP's struct type) is assigned by a 16-byte memcpy, and in the re-run
 * kernel -- one load path, no cooperative alternative -- those memcpys survived the optimiser as they were: global -> private
 * memory -> LDS, i.e. the sets lived in scratch (272 bytes per lane; r04: 576 with the states) and every block of loads had to
 * ARRIVE before it could be put away, which is the opposite of a prefetch */
typedef float wm_f4 __attribute__((vector_size(16)));

/* a value every lane of the wave holds alike, moved to scalar registers */
__device__ __forceinline__ uint32_t wm_uniform(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}
__device__ __forceinline__ uint64_t wm_uniform64(uint64_t v) { return ((uint64_t)wm_uniform((uint32_t)(v >> 32)) << 32) | wm_uniform((uint32_t)v); }

#if defined(__HIP_DEVICE_COMPILE__)
#define WM_CLK_ANY(p) (__ballot(p) != 0ull)      /* "some lane of the wave still has a chip in this block": an early exit, never a decision */
#else
#define WM_CLK_ANY(p) true
#endif

#define WM_CLK_XROW 36           /* words per lane in the soft-symbol rows: 32 + 4 (rows stay 16-byte aligned; a lane's 8 ds_read_b128
                                    are bank-conflict free: 9 L mod 16 is a permutation) */
#define WM_CLK_CROW 17           /* words per lane in the chip staging (16 + 1) */
#define WM_CLK_BROW 9            /* words per lane in the one-wave form's slicer-word staging (8 + 1) */
#define WM_CLK_SR_WINDOW 1024u   /* samples before a segment over which a warm-up keeps the time2 shift register (clk_warm_chips) */

struct IirCoef { float a1[3], a2[3], b1[3], b2[3]; };

__device__ __forceinline__ IirCoef iir_coef(uint32_t ch)
{
    IirCoef c;
    if (ch == 0) { /* rtl_wmbus.c:340-341 */
        c.b1[0] = 1.999994649f; c.b2[0] = 0.9999946492f; c.b1[1] = -1.99999482f; c.b2[1] = 0.9999948196f;
        c.b1[2] = 1.703868036e-07f; c.b2[2] = -1.000010531f;
        c.a1[0] = -1.387139203f; c.a2[0] = 0.9921518712f; c.a1[1] = -1.403492665f; c.a2[1] = 0.9845934971f;
        c.a1[2] = -1.430055639f; c.a2[2] = 0.9923856172f;
    } else {       /* rtl_wmbus.c:355-356 */
        c.b1[0] = 1.999994187f; c.b2[0] = 0.9999941867f; c.b1[1] = -1.999994026f; c.b2[1] = 0.9999940262f;
        c.b1[2] = -1.605750097e-07f; c.b2[2] = -1.000011787f;
        c.a1[0] = -1.92151475f; c.a2[0] = 0.9918135499f; c.a1[1] = -1.922481015f; c.a2[1] = 0.984593497f;
        c.a1[2] = -1.937432099f; c.a2[2] = 0.9927241336f;
    }
    return c;
}

/* one sample through section K (iir.h:57-74; b0 == 1) */
template <int K>
__device__ __forceinline__ float clk_biquad(float v, float &h1, float &h2, const IirCoef &c)
{
    const float h0 = wm_sub(v, wm_add(wm_mul(c.a1[K], h1), wm_mul(c.a2[K], h2)));
    const float o = wm_add(wm_add(h0, wm_mul(c.b1[K], h1)), wm_mul(c.b2[K], h2));
    h2 = h1; h1 = h0;
    return o;
}

/* One sample through DC remover + squarer + 3 biquads; returns the clock level (iir.h:57-74). */
__device__ __forceinline__ bool clk_step(WmClkState &s, const IirCoef &c, bool dc, float x, float &soft)
{
    if (dc) { /* rtl_wmbus.c:501/511: (1+a)/2 * (x - x_old) + a * y_old, a = 0.999f */
        const float al = 0.999f, k = wm_div(wm_add(1.0f, al), 2.0f);
        const float y = wm_add(wm_mul(k, wm_sub(x, s.dc_x)), wm_mul(al, s.dc_y));
        s.dc_x = x; s.dc_y = y; x = y;
    }
    soft = x;
    float v = wm_mul(x, x);
    v = clk_biquad<0>(v, s.h[0], s.h[1], c);
    v = clk_biquad<1>(v, s.h[2], s.h[3], c);
    v = clk_biquad<2>(v, s.h[4], s.h[5], c);
    return wm_mul(v, 1.874981046e-06f) >= 0.0f;
}

/* A lane state as its twelve words, and two states compared bit for bit -- member by member: viewing the struct through a
 * uint32_t pointer makes the compiler keep it in memory (scratch) in the re-run kernel, whose chain walk carries a state from
 * one segment into the next (round 4: 576 bytes of scratch per lane, sixteen scratch accesses inside the 32-sample block loop). */
__device__ __forceinline__ void clk_state_words(const WmClkState &s, uint32_t (&w)[12])
{
#pragma unroll
    for (int i = 0; i < 6; i++) w[i] = wm_f2u(s.h[i]);
    w[6] = wm_f2u(s.dc_x); w[7] = wm_f2u(s.dc_y); w[8] = s.clk; w[9] = s.sr; w[10] = s.pad[0]; w[11] = s.pad[1];
}
__device__ __forceinline__ bool clk_state_same(const WmClkState &a, const WmClkState &b)
{
    uint32_t x[12], y[12];
    clk_state_words(a, x); clk_state_words(b, y);
    bool same = true;
#pragma unroll
    for (int i = 0; i < 12; i++) same &= x[i] == y[i];
    return same;
}

/* Clock lock.  The reference's lock counter (rtl_wmbus.c:1092-1111: rising edge -> 1, still high -> 2, third high sample -> take the
 * bit) is equivalent to "sample at n iff the clock levels at n-3 .. n are L,H,H,H" (checked exhaustively over all level sequences,
 * DESIGN.md).  low: the 32 levels of a block as wm_shift_in_level_low collected them; clk: the last three levels before the block,
 * newest in bit 0 (WmClkState.clk), replaced by the block's last three.  Returns the block's sample mask (bit n: take the bit at n). */
__device__ __forceinline__ uint32_t clk_lock_mask(const uint32_t low, uint32_t &clk)
{
    const uint32_t prev3 = ((clk & 1u) << 2) | (clk & 2u) | ((clk >> 2) & 1u);              /* here time runs upwards */
    const uint64_t H = ((uint64_t)(~__builtin_bitreverse32(low)) << 3) | prev3;           /* bit n+3 = level at n */
    const uint32_t last3 = (uint32_t)(H >> 32) & 7u;                                        /* levels at 29, 30, 31 */
    clk = ((last3 & 1u) << 2) | (last3 & 2u) | ((last3 >> 2) & 1u);
    return (uint32_t)((~H) & (H >> 1) & (H >> 2) & (H >> 3));
}

/* the time2 framer's access code of a chain, and whether time2 chips are wanted at all */
struct ClkSync { uint32_t word, mask; bool t2a; };
__device__ __forceinline__ ClkSync clk_sync(const K2Args &a, const uint32_t ch)
{
    return ClkSync{ch ? WM_SYNC_S1 : WM_SYNC_T1C1, ch ? WM_SYNC_S1_MASK : WM_SYNC_T1C1_MASK, (a.g.flags & WM_F_T2A) != 0u};
}

/* ---- a segment's geometry and the state its walk starts from ---------------------------------------------------------------------- */
struct ClkGeo {
    uint64_t row, sidx;              /* (chain, capture); its segment's records */
    uint32_t mb, me, me_full;        /* the lane's samples [mb, me); whole 32-sample blocks end at me_full */
    uint32_t m0, nb;                 /* first sample of the lane's walk (warm-up start), number of whole blocks of the walk */
};

/* span: segments the lane covers (2: the one-wave form's S1 lanes under WmPush.s1_span).  A re-run starts at the segment, from an
 * exact state; the first pass starts warm[ch] samples early from the all-zero state, or at the push start from the carried one. */
__device__ __forceinline__ ClkGeo clk_geo(const K2Args &a, const bool rerun, const uint32_t ch, const uint32_t stream, const uint32_t seg, const uint32_t span = 1u)
{
    const WmPush &g = a.g;
    ClkGeo G;
    G.row = (uint64_t)ch * g.S + stream; G.sidx = G.row * g.nseg_cap[1] + seg;
    G.mb = seg * g.seg_len[1]; G.me = min(g.M, G.mb + span * g.seg_len[1]);
    G.me_full = G.mb + ((G.me - G.mb) & ~31u);
    const uint32_t w = g.warm[ch];
    G.m0 = rerun ? G.mb : (G.mb <= w ? 0u : G.mb - w);
    G.nb = (G.me_full - G.m0) >> 5;
    return G;
}
__device__ __forceinline__ WmClkState clk_start_state(const K2Args &a, const ClkGeo &G, const bool rerun, const uint32_t ch, const uint32_t seg)
{
    const WmClkState *stF = (const WmClkState *)a.st_final, *stC = (const WmClkState *)a.st_carry;
    if (rerun) return seg ? stF[G.sidx - 1u] : stC[G.row];       /* the predecessor's end state as recorded / the carried state */
    if (G.mb <= a.g.warm[ch]) return stC[G.row];                 /* exact: the walk starts at the push start */
    return WmClkState{};                                         /* speculative cold start */
}
/* a warm-up block whose chips nobody looks at: it ends more than WM_CLK_SR_WINDOW samples before the segment, so the recurrences run
 * as ever and what only feeds the output is left out (the WARM variants of the forms' block functions) */
__device__ __forceinline__ bool clk_warm_short(const uint32_t mb, const uint32_t m) { return m < mb && mb - m > WM_CLK_SR_WINDOW + 32u; }

/* ---- soft symbols: memory -> a register set -> the LDS rows ------------------------------------------------------------------------
 * A lane walks its own row (chain, capture) of soft symbols, 128 bytes per 32-sample block.  When the 64 lanes of a wave are 64
 * consecutive captures of one (chain, segment) in lock step -- first pass, n_streams a multiple of 64 -- the wave fetches the 64 rows'
 * blocks COOPERATIVELY: lane ln fetches piece ln % 8 of row (row0 + 8 i + ln / 8), i = 0 .. 7, so 8 lanes read one whole 128-byte
 * line, and the block is transposed through LDS (conflict-free, see WM_CLK_XROW).  Eight addresses = a UNIFORM base (row0 + 8 i and the
 * sample index: scalar registers) + one 32-bit lane offset.  Lane-private 16-byte loads of the same data touch 64 lines per
 * instruction and re-fetch each line from L2 several times; re-run launches and odd capture counts take them. */
struct ClkLoad {
    const float *xown;               /* lane-private: my row */
    uint64_t crow0;                  /* cooperative: first row of the wave (uniform) */
    uint32_t coff;                   /* cooperative: my piece's offset from the start of row crow0 + 8 i */
    uint32_t m_last;                 /* the last whole block: requests past it are clamped into the segment */
    uint32_t xw, xw_step;            /* where my eight pieces go in the rows (coop: other lanes' rows; else my own) */
};
__device__ __forceinline__ void clk_load_segment(ClkLoad &L, const K2Args &a, const ClkGeo &G, const uint32_t ln)
{
    L.xown = a.dphi + G.row * a.g.Mcap;
    L.crow0 = wm_uniform64(G.row - ln);
    L.m_last = G.me_full >= 32u ? G.me_full - 32u : 0u;
}
__device__ __forceinline__ ClkLoad clk_load_init(const K2Args &a, const ClkGeo &G, const bool coop, const uint32_t ln)
{
    ClkLoad L;
    clk_load_segment(L, a, G, ln);
    L.coff = (ln >> 3) * a.g.Mcap + 4u * (ln & 7u);
    L.xw = coop ? (ln >> 3) * WM_CLK_XROW + 4u * (ln & 7u) : ln * WM_CLK_XROW;
    L.xw_step = coop ? 8u * WM_CLK_XROW : 4u;
    return L;
}
__device__ __forceinline__ void clk_fetch(const K2Args &a, const ClkLoad &L, const bool coop, wm_f4 (&gx)[8], uint32_t mm)
{
    mm = min(mm, L.m_last);
    if (coop) {
        const uint32_t mu = wm_uniform(mm);
#pragma unroll
        for (int i = 0; i < 8; i++) gx[i] = *(const wm_f4 *)(a.dphi + ((L.crow0 + 8u * i) * a.g.Mcap + mu) + L.coff);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) gx[i] = *(const wm_f4 *)(L.xown + mm + 4 * i);
    }
}
/* a fetched block -> the lanes' rows; the rows' previous block has been read (coop: by every lane of the wave) */
__device__ __forceinline__ void clk_stage(const ClkLoad &L, const bool coop, float *rows, const wm_f4 (&gx)[8])
{
    if (coop) __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 8; i++) *(wm_f4 *)(rows + L.xw + i * L.xw_step) = gx[i];
    if (coop) __builtin_amdgcn_wave_barrier();
}

/* ---- the chips of a 32-sample block (rtl_wmbus.c:818-828): at most 8, because the lock pattern needs 4 samples; oldest first; the wave
 * stops as soon as none of its lanes has a chip left (T1/C1 lanes meet 4 per block, S1 lanes 1.3: half the trips of the fixed eight) - */
/* Warm-up block at `ahead` = mb - m samples before the segment: shift-register upkeep only.  The register is a function of the last
 * 16 / 24 chips, so the upkeep starts WM_CLK_SR_WINDOW samples before the segment (>= 40 chips of either chain at their nominal rates;
 * if a stretch of silence leaves fewer, the hand-off does not certify and the segment is re-run, as after any other uncertified start) */
__device__ __forceinline__ void clk_warm_chips(uint32_t &sr, uint32_t smask, const uint32_t bitw, const ClkSync &y, const uint32_t ahead)
{
    if (ahead > WM_CLK_SR_WINDOW) smask = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const bool has = smask != 0u;
        if (!WM_CLK_ANY(has)) break;
        const uint32_t k = has ? (uint32_t)__ffs((int)smask) - 1u : 0u;
        smask &= smask - 1u;
        const uint32_t sr_new = ((sr << 1) | ((bitw >> k) & 1u)) & y.mask;
        sr = has ? sr_new : sr;
    }
}
/* Block of the segment proper, `rel` = m - mb samples into it: trip i's chip word goes to slot(i), the caller's staging (slots beyond
 * the block's chips are written too and rewritten by the next block).  Returns the number of chips. */
template <class Slot>
__device__ __forceinline__ uint32_t clk_block_chips(uint32_t &sr, uint32_t &saw_sync, uint32_t smask, const uint32_t bitw, const ClkSync &y, const uint32_t rel, Slot slot)
{
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const bool has = smask != 0u;
        if (!WM_CLK_ANY(has)) break;
        const uint32_t k = has ? (uint32_t)__ffs((int)smask) - 1u : 0u;
        smask &= smask - 1u;
        const uint32_t bit = (bitw >> k) & 1u;
        const uint32_t sr_new = ((sr << 1) | bit) & y.mask;
        sr = has ? sr_new : sr;
        const uint32_t val = bit | (sr_new == y.word ? 2u : 0u);
        saw_sync |= has ? (val & 2u) : 0u;
        slot(i) = WM_CHIP_WORD(rel + k, val);
        cnt += has;
    }
    return cnt;
}

/* ---- slicer words (one per 32 samples and lane) leave in whole, 32-byte aligned groups of 8, like the chips (see k2_rla: partial-sector
 * stores from 131 072 lanes with private output regions become read-modify-write traffic).  stage: the lane's eight staging words in
 * LDS, `stride` words apart; bi: the block's index in the row.  Returns whether the group left. */
__device__ __forceinline__ bool clk_bits_put(uint32_t *bw, uint32_t *stage, const uint32_t stride, const uint32_t bi, const uint32_t bitw)
{
    stage[(bi & 7u) * stride] = bitw;
    if ((bi & 7u) != 7u) return false;
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = stage[i * stride];
    *(uint4 *)(bw + (bi - 7u)) = make_uint4(w[0], w[1], w[2], w[3]);
    *(uint4 *)(bw + (bi - 3u)) = make_uint4(w[4], w[5], w[6], w[7]);
    return true;
}
/* the incomplete last group of a walk whose whole blocks end at block index `end` */
__device__ __forceinline__ void clk_bits_rest(uint32_t *bw, const uint32_t *stage, const uint32_t stride, const uint32_t end)
{
    for (uint32_t bi = end & ~7u; bi < end; bi++) bw[bi] = stage[(bi & 7u) * stride];
}

/* ---- interior checkpoint j of a segment: RECORDED by the first pass (lane state s, chips so far), MET again by a re-run.
 * ck: the segment's checkpoint records, nck of them; out: its chip region, of which n_fl chips are in memory and `pend` more wait in
 * the caller's staging (pending(i), i < pend).  Returns true when the lane leaves here. */
template <class Pending>
__device__ __forceinline__ bool clk_checkpoint(const K2Args &a, const bool rerun, const WmClkState &s, uint32_t *ck, const uint32_t j, const uint32_t nck, const uint64_t sidx,
                                               uint32_t *out, const uint32_t n_fl, const uint32_t pend, const uint32_t saw_sync, Pending pending)
{
    uint32_t *q = ck + 16u * j;
    uint32_t sw[12];
    clk_state_words(s, sw);
    const uint32_t n1 = n_fl + pend;
    if (rerun) {
        bool same = true;
#pragma unroll
        for (int i = 0; i < 12; i++) same &= q[i] == sw[i];
        const uint32_t n0 = q[12];
        if (same && n1 <= n0) {
            /* Back on the speculative pass's trajectory: everything it produced from here on is exact already.  My chips replace its
             * first n0; if they are fewer, its tail moves down.  (More chips than it had: its tail is partly overwritten -- run on to
             * the segment's end.) */
            for (uint32_t i = 0; i < pend; i++) out[n_fl + i] = pending(i);
            if (n1 < n0) {
                const uint32_t total0 = a.counts[sidx];
                for (uint32_t i = n0; i < total0; i++) { const uint32_t w = out[i]; out[n1 + (i - n0)] = w; }
                a.counts[sidx] = n1 + (total0 - n0);
                /* this and the later checkpoints describe the tail, which has moved: a later round may re-run this segment again
                 * and meet them */
                for (uint32_t jj = j; jj < nck; jj++) ck[16u * jj + 12u] -= n0 - n1;
            }
            if (saw_sync) a.sync_seen[sidx] = 1u;       /* the tail's flag, if any, is already set */
            return true;
        }
        /* Not on the recorded trajectory: from here on the region holds MY chips (and all of it if I run to the end), so the checkpoint
         * must describe me -- a later round that re-runs this segment once more compares against what is in memory, not against the
         * speculative pass.  (Found by the randomised tests: two chips lost after a second round met a checkpoint whose chip count
         * predated the first round's move.) */
    }
    *(uint4 *)(q) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
    *(uint4 *)(q + 4) = make_uint4(sw[4], sw[5], sw[6], sw[7]);
    *(uint4 *)(q + 8) = make_uint4(sw[8], sw[9], sw[10], sw[11]);
    q[12] = n1;
    return false;
}

/* ---- the end of a segment whose whole blocks are done: s = the state after the last of them, n_out = the chips so far (all in
 * memory).  The ragged tail of a row's last segment sample by sample, its chips, then the end record (at sidx_end: the lane's last
 * segment), the count (cap_t2: the lane's chip region), the access-code flag. */
template <bool DC>
__device__ __forceinline__ void clk_segment_end(const K2Args &a, const ClkGeo &G, const IirCoef &c, const ClkSync &y, WmClkState &s, uint32_t *out, uint32_t *bw,
                                                uint32_t n_out, uint32_t saw_sync, const uint32_t cap_t2, const uint64_t sidx_end)
{
    if (G.me_full < G.me) {
        const float *x = a.dphi + G.row * a.g.Mcap;
        const uint32_t m = G.me_full;
        uint32_t bitw = 0, smask = 0, hist = s.clk;
        for (uint32_t k = 0; m + k < G.me; k++) {
            float soft;
            const uint32_t high = clk_step(s, c, DC, x[m + k], soft);
            hist = ((hist << 1) | high) & 0xFu;
            bitw |= (uint32_t)(soft >= 0.0f) << k;
            smask |= (uint32_t)(hist == 7u) << k;
        }
        s.clk = hist & 7u;
        bw[m >> 5] = bitw;
        while (smask) {                                  /* rtl_wmbus.c:818-828 */
            const uint32_t k = (uint32_t)__ffs((int)smask) - 1u;
            smask &= smask - 1u;
            const uint32_t bit = (bitw >> k) & 1u;
            s.sr = ((s.sr << 1) | bit) & y.mask;
            if (y.t2a) {
                const uint32_t val = bit | (s.sr == y.word ? 2u : 0u);
                saw_sync |= val & 2u;
                if (n_out < cap_t2) out[n_out] = WM_CHIP_WORD(m + k - G.mb, val);
                n_out++;
            }
        }
    }
    ((WmClkState *)a.st_final)[sidx_end] = s;
    a.counts[G.sidx] = min(n_out, cap_t2);
    if (saw_sync) a.sync_seen[G.sidx] = 1u;
    if (n_out > cap_t2) atomicOr(a.err, WM_ERR_CHIP_OVERFLOW);       /* cannot happen: the lock pattern takes >= 4 samples per chip */
}

/* ---- chain walk of a re-run lane (from the SECOND list round on; K2Args.bad set).  A segment is listed because its start did not match
 * its predecessor's end; k2_verify also leaves that verdict per segment in `a.bad`.  The first list round re-runs every listed segment on
 * its own, in parallel, from the predecessor's end state as recorded -- right unless that predecessor is itself re-run and comes out
 * different, which is rare with whole-wave batches (fewer than ten lanes of 16 384) and the rule with the short segments of a small
 * batch, where a slowly converging stretch covers several segments and every round settled one more of them (a single capture of
 * configs[1] fell to the host-driven path on every push).  In a chain walk the FIRST listed segment of a run of consecutive listed ones
 * does them all, one after the other, each from the exact end state of the one before (the others return at once), and goes on into the
 * segment behind the run as long as the end state it arrives with differs from that segment's recorded start -- unless that segment has
 * a lane of its own in this launch (listed behind an unlisted one), which the next round sorts out.  (Walking chains already in the
 * first list round made it 2.8 ms longer on the bench workload: neighbours that are both listed usually both leave at an early
 * checkpoint, and serialising them doubles the longest lane.) */
__device__ __forceinline__ const uint32_t *clk_verdicts(const K2Args &a, const uint32_t ch, const uint32_t stream)
{
    return a.bad + (uint64_t)ch * a.g.nseg_cap[1] * a.g.S + stream;                  /* verdict of segment j at [j * S] */
}
/* the head of my run of listed segments covers me */
__device__ __forceinline__ bool clk_chain_covered(const K2Args &a, const uint32_t *bad, const uint32_t seg) { return seg > 0u && bad[(uint64_t)(seg - 1u) * a.g.S] != 0u; }
/* Segment seg (records at sidx) is done: met = it left at a checkpoint, so the recorded end state was exact already and replaces fin;
 * else fin is its end state.  Returns true when the lane goes on into segment seg + 1, from fin. */
__device__ __forceinline__ bool clk_chain_next(const K2Args &a, const uint32_t *bad, const bool met, const uint32_t seg, const uint64_t sidx, WmClkState &fin)
{
    const WmClkState *stS = (const WmClkState *)a.st_start, *stF = (const WmClkState *)a.st_final;
    if (met) fin = stF[sidx];
    if (seg + 1u >= a.g.nseg[1]) return false;
    const WmClkState next = stS[sidx + 1u];
    if (clk_state_same(fin, next)) return false;             /* the next segment started from exactly this state */
    if (bad[(uint64_t)(seg + 1u) * a.g.S] && !bad[(uint64_t)seg * a.g.S]) return false;      /* it is listed and has a lane of its own in this launch: next round */
    return true;
}

#endif /* WM_K2_CLOCK_LANE_H */
