/* wm_k3_repair.h -- cfg.crc_repair: a time2 telegram that k3_bursts has decoded whole inside the push and that fails a block CRC is
 * repaired by flipping its least reliable chips (the rule: include/wmbus_hip.h, CRC REPAIR; tests/repair_ref.py restates it).  Device
 * code, included by wm_kernels.hip behind wm_k3_levels.h: it runs behind k3_bursts and the level stage, on their records. */
#ifndef WM_K3_REPAIR_H
#define WM_K3_REPAIR_H

#define WM_REP_K        8u         /* candidates per bad block: 255 patterns */
#define WM_REP_MAXCHIPS 1024u      /* chips of the longest block: 128 bytes of a C1 frame B */

typedef wmbus_repair WmRepair;     /* the kernel writes the very records wmbus_line_repairs() hands out */

struct K3RepArgs {
    K3Args k3;                   /* what k3_bursts ran with: the chip regions, and the packets and the byte arena it has just written */
    const float *dphi;           /* [2][S][Mcap] this push's soft symbols */
    const float *tail_in;        /* [2 S][WM_LEV_TAIL] the soft symbols in front of this push (K3LevArgs.tail_in) */
    const uint2 *src_pkts;       /* K3Args.lev_pkt: {the access-code chip's sample within the push, row} per packet slot */
    WmRepair *rep_pkts;          /* [pkts_cap] pinned host memory: record i belongs to packet i */
};

/* Per-wave scratch: the telegram's chips as a bit string (chip j = bit j % 64 of word j / 64, as in k3_bursts) and the keys
 * r << 10 | (chip within the block) of one block's chips. */
struct K3RepLds { unsigned long long bits[4][WM_K3_BITWORDS]; uint32_t key[4][WM_REP_MAXCHIPS]; };

__device__ __forceinline__ uint32_t rep_wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

/* Byte b of the telegram from the bit string, its chips XORed with `flip` (first chip of the byte in the field's most significant
 * bit); bit 8 of the result: a symbol (T1) or a pair (S1) of the byte is no code word.  mode: 0 T1, 1 C1, 2 S1. */
__device__ __forceinline__ uint32_t rep_byte(const unsigned long long *bits, uint32_t mode, uint32_t b, uint32_t flip)
{
    if (mode == 0u) {
        const uint32_t f = k3_field(bits, 1u + 12u * b, 12) ^ flip;
        const uint32_t hi = D3OF6[f >> 6], lo = D3OF6[f & 63u];
        return (hi == 255u || lo == 255u) ? 0x1FFu : (hi << 4) | lo;
    }
    if (mode == 1u) return k3_field(bits, 17u + 8u * b, 8) ^ flip;
    const uint32_t sym = k3_field(bits, 1u + 16u * b, 16) ^ flip;
    uint32_t v = 0, bad = 0;
#pragma unroll
    for (int q = 7; q >= 0; q--) {
        const uint32_t pair = (sym >> (2 * q)) & 3u;
        bad |= (pair == 0u || pair == 3u);
        v = (v << 1) | (pair == 1u);
    }
    return v | (bad << 8);
}

__device__ __forceinline__ uint32_t rep_crc_step(uint32_t crc, uint32_t byte)
{
    crc ^= byte << 8;
#pragma unroll
    for (int k = 0; k < 8; k++) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x3D65u) : (crc << 1);
    return crc & 0xFFFFu;
}

/* Is the block [start, start + blk) of the telegram in the bit string clean?  By one lane. */
__device__ __forceinline__ bool rep_block_clean(const unsigned long long *bits, uint32_t mode, uint32_t start, uint32_t blk)
{
    if (blk < 2u) return false;
    uint32_t crc = 0;
    for (uint32_t b = 0; b + 2u < blk; b++) crc = rep_crc_step(crc, rep_byte(bits, mode, start + b, 0u) & 255u);
    return ((~crc) & 0xFFFFu) == (((rep_byte(bits, mode, start + blk - 2u, 0u) & 255u) << 8) | (rep_byte(bits, mode, start + blk - 1u, 0u) & 255u));
}

/* One packet record, by one wave. */
__device__ void repair_item(const K3RepArgs &a, const uint32_t slot, const uint32_t ln, unsigned long long *s_bits, uint32_t *s_key)
{
    const WmPush &g = a.k3.g;
    WmRepair rec = {};
    const WmPkt p = a.k3.pkts[slot];
    /* the subject: a time2 telegram, complete, not clean, long enough to have a CRC verdict at all.  (An S1 telegram with an invalid
     * Manchester pair never got here: it is an ABORT.) */
    const bool subject = p.status == WM_PKT_DONE && p.algo == 1u && !(p.flags & WM_PKTF_CRC_OK) && p.L >= 12u && p.L <= WM_PKT_MAXBYTES &&
                         p.stream < g.S && p.chain < 2u;
    if (!subject) { if (ln == 0) a.rep_pkts[slot] = rec; return; }
    const uint32_t mode = p.chain ? 2u : (p.flags & WM_PKTF_C1) ? 1u : 0u, frame_b = (p.flags & WM_PKTF_FRAME_B) ? 1u : 0u, L = p.L;
    const uint32_t cpb = mode == 0u ? 12u : mode == 1u ? 8u : 16u, off = mode == 1u ? 17u : 1u;
    const uint32_t n = off + cpb * L;                        /* the chips the decoder took, the access-code chip included */

    /* ---- the chips again: the access-code chip's segment from its sample, its index there from the counts in front of it ---- */
    K3Item it;
    it.algo = 1u; it.ch = p.chain; it.stream = p.stream; it.cont = 0;
    it.nseg = g.nseg[1]; it.seg_len = g.seg_len[1];
    it.row = (uint64_t)it.ch * g.S + it.stream;
    it.cnt = a.k3.counts[1] + it.row * g.nseg_cap[1];
    it.sidx0 = it.row * g.nseg_cap[1];
    const uint32_t rel = a.src_pkts[slot].x;                 /* the access-code chip's sample within the push */
    it.seg = min(rel / it.seg_len, it.nseg - 1u);
    uint32_t before = 0, total = 0;
    for (uint32_t s = ln; s < it.nseg; s += 64u) { const uint32_t c = it.cnt[s]; if (s < it.seg) before += c; total += c; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o); total += __shfl_xor(total, o); }
    /* what k3_bursts decoded lies inside the push's chip stream; anything else is not this kernel's to touch */
    if (p.chip0 < before || p.chip0 >= total || total - p.chip0 < n || rel >= g.M) { if (ln == 0) a.rep_pkts[slot] = rec; return; }
    it.k = p.chip0 - before; it.chip0 = p.chip0; it.avail = total - p.chip0; it.n = n;

    for (uint32_t j0 = 0; j0 < n; j0 += 64u) {
        const uint32_t j = j0 + ln;
        uint32_t w = 0;
        if (j < n) { uint32_t sg, kk; k3_locate(it, j, sg, kk); w = k3_chip(a.k3, it, sg, kk); }
        const unsigned long long m = __ballot(w & 1u);
        if (ln == 0) s_bits[j0 >> 6] = m;
    }
    if (ln == 0) s_bits[(n + 63u) >> 6] = 0ull;              /* k3_field may look one word ahead */
    WM_WAVE_SYNC();

    /* ---- c: LINE LEVELS' mean over the preamble window, 0 where that record is invalid ---- */
    int32_t c = 0;
    {
        const uint32_t lo = p.chain ? WM_LEV_LO_S : WM_LEV_LO_T, hi = p.chain ? WM_LEV_HI_S : WM_LEV_HI_T, N = lo - hi;
        if (g.m0 + rel >= lo) {
            const float *now = a.dphi + it.row * g.Mcap, *front = a.tail_in + it.row * WM_LEV_TAIL + WM_LEV_TAIL;
            const int32_t w0 = (int32_t)rel - (int32_t)lo;   /* >= -WM_LEV_TAIL */
            int32_t sum = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint32_t j = ln + 64u * (uint32_t)t;
                if (j < N) { const int32_t m = w0 + (int32_t)j; sum += lev_quant(m >= 0 ? now[m] : front[m]); }
            }
            sum = lev_wave_sum(sum);
            c = (int32_t)lev_floordiv(2 * (int64_t)sum + N, 2 * (int64_t)N);
        }
    }

    /* ---- the bad blocks: lane i checks block i (frame A of 290 bytes has 17, frame B of 256 two) ---- */
    const uint32_t first = frame_b ? 128u : 12u, next = frame_b ? 128u : 18u;
    unsigned long long bad_mask;
    {
        const uint32_t start = ln == 0 ? 0u : first + (ln - 1u) * next;
        bool bad = false;
        if (start < L) bad = !rep_block_clean(s_bits, mode, start, min(ln == 0 ? first : next, L - start));
        bad_mask = __ballot(bad);
    }
    uint32_t n_bad = 0, n_rep = 0, n_flip = 0, weight = 0;
    for (unsigned long long todo = bad_mask; todo; todo &= todo - 1ull) {
        const uint32_t bi = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t start = bi == 0u ? 0u : first + (bi - 1u) * next, blk = min(bi == 0u ? first : next, L - start);
        n_bad++;
        const uint32_t nch = cpb * blk, jlo = off + cpb * start, excl = start == 0u ? cpb : 0u;      /* the L-field byte's chips are no candidates */
        if (blk < 3u || nch > WM_REP_MAXCHIPS) continue;
        /* keys of the block's chips: r << 10 | index within the block (r <= 2^21: below 2^32 - 1), ~0 for a chip that is no candidate */
        for (uint32_t t0 = 0; t0 < nch; t0 += 64u) {
            const uint32_t t = t0 + ln;
            if (t < nch) {
                uint32_t key = 0xFFFFFFFFu;
                if (t >= excl) {
                    uint32_t sg, kk; k3_locate(it, jlo + t, sg, kk);
                    const uint32_t pm = sg * it.seg_len + WM_CHIP_POS(k3_chip(a.k3, it, sg, kk));
                    const int32_t q = pm < g.M ? lev_quant(a.dphi[it.row * g.Mcap + pm]) : 0;
                    const int32_t r = q >= c ? q - c : c - q;
                    key = ((uint32_t)r << 10) | t;
                }
                s_key[t] = key;
            }
        }
        WM_WAVE_SYNC();
        /* the K smallest (r, j), ascending: K wave-wide minima over the keys above the one before */
        const uint32_t K = min(WM_REP_K, nch - excl);
        uint32_t cand[WM_REP_K];
        uint32_t prev = 0;
#pragma unroll
        for (uint32_t i = 0; i < WM_REP_K; i++) {
            uint32_t best = 0xFFFFFFFFu;
            if (i < K)
                for (uint32_t t = ln; t < nch; t += 64u) { const uint32_t key = s_key[t]; if ((i == 0u || key > prev) && key < best) best = key; }
            best = rep_wave_min(best);
            cand[i] = best; prev = best;
        }
        /* the patterns over the lanes: m = 1 ... 2^K - 1, valid where every byte is a code word and the CRC is right; key (w, m) */
        unsigned long long best = ~0ull;
        for (uint32_t m = ln + 1u; m < (1u << K); m += 64u) {
            unsigned long long w = 0;
            uint32_t cbyte[WM_REP_K], cflip[WM_REP_K];       /* per candidate: its byte within the block, its bit in that byte's field */
#pragma unroll
            for (uint32_t i = 0; i < WM_REP_K; i++) {
                const uint32_t t = cand[i] & 1023u, on = i < K && ((m >> i) & 1u);
                cbyte[i] = on ? t / cpb : 0xFFFFFFFFu;
                cflip[i] = 1u << (cpb - 1u - t % cpb);
                if (on) w += cand[i] >> 10;
            }
            uint32_t crc = 0, invalid = 0, tail2 = 0;
            for (uint32_t b = 0; b < blk; b++) {
                uint32_t flip = 0;
#pragma unroll
                for (uint32_t i = 0; i < WM_REP_K; i++) flip ^= cbyte[i] == b ? cflip[i] : 0u;
                const uint32_t v = rep_byte(s_bits, mode, start + b, flip);
                invalid |= v >> 8;
                if (b + 2u < blk) crc = rep_crc_step(crc, v & 255u);
                else tail2 = (tail2 << 8) | (v & 255u);
            }
            if (!invalid && ((~crc) & 0xFFFFu) == tail2) { const unsigned long long key = (w << 8) | m; best = key < best ? key : best; }
        }
        {
            uint32_t bh = (uint32_t)(best >> 32), bl = (uint32_t)best;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const uint32_t oh = __shfl_xor(bh, o), ol = __shfl_xor(bl, o);
                if (oh < bh || (oh == bh && ol < bl)) { bh = oh; bl = ol; }
            }
            best = ((unsigned long long)bh << 32) | bl;
        }
        if (best != ~0ull) {
            const uint32_t m = (uint32_t)best & 255u;
            n_rep++; n_flip += (uint32_t)__popc(m); weight += (uint32_t)(best >> 8);
            if (ln == 0) {                                   /* the repair goes into the bit string: blocks do not share chips */
#pragma unroll
                for (uint32_t i = 0; i < WM_REP_K; i++)
                    if (i < K && ((m >> i) & 1u)) { const uint32_t j = jlo + (cand[i] & 1023u); s_bits[j >> 6] ^= 1ull << (j & 63u); }
            }
        }
        WM_WAVE_SYNC();                                      /* the keys are reused by the next block */
    }

    /* ---- all or nothing: the repaired bytes into the packet's own slot of the arena, the flags as if these chips had been decoded ---- */
    if (n_rep == n_bad && n_bad != 0u) {
        uint32_t err36 = 0;
        for (uint32_t b = ln; b < L; b += 64u) {
            const uint32_t v = rep_byte(s_bits, mode, b, 0u);
            err36 |= v >> 8;
            a.k3.bytes[p.off + b] = (uint8_t)v;
        }
        err36 = mode == 0u && __ballot(err36) != 0ull;
        if (ln == 0) a.k3.pkts[slot].flags = (uint8_t)((p.flags & ~(uint32_t)WM_PKTF_ERR3OF6) | (err36 ? WM_PKTF_ERR3OF6 : 0u) | WM_PKTF_CRC_OK);
    }
    rec.blocks_bad = (uint16_t)n_bad; rec.blocks_repaired = (uint16_t)n_rep; rec.chips_flipped = (uint16_t)n_flip; rec.weight = weight;
    if (ln == 0) a.rep_pkts[slot] = rec;
    WM_WAVE_SYNC();                                          /* the scratch is reused by the wave's next record */
}

/* Behind k3_bursts and the level stage, on the packet records: as few blocks as those kernels, for the same reason (a latency-bound
 * wave parked on a SIMD costs the demodulation kernel a wave slot there, see k3_bursts).  A wave returns at once from a record that is
 * no subject, and subjects are the exception. */
__global__ __launch_bounds__(256) void k3_repair(K3RepArgs a)
{
    wm_framer_prio();
    __shared__ K3RepLds lds;
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t np = min(*a.k3.n_pkts, a.k3.pkts_cap);
    for (uint32_t r = blockIdx.x * 4u + wv; r < np; r += gridDim.x * 4u) repair_item(a, r, ln, lds.bits[wv], lds.key[wv]);
}

#endif /* WM_K3_REPAIR_H */
