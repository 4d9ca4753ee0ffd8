/* wm_k3_rescue.h -- cfg.s1_rescue: an S1 telegram of the time2 framer that k3_bursts has aborted at an invalid Manchester pair, and
 * whose chips lie whole inside the push, is decoded again with every invalid pair decided by its two soft symbols (the rule:
 * include/wmbus_hip.h, S1 RESCUE; tests/rescue_ref.py restates it).  Device code, included by wm_kernels.hip behind wm_k3_repair.h: it
 * runs behind k3_bursts and the level stage, on their records, and before the packet counters and the byte count go to the host. */
#ifndef WM_K3_RESCUE_H
#define WM_K3_RESCUE_H

typedef wmbus_rescue WmRescue;     /* the kernel writes the very records wmbus_line_rescues() hands out */

#define WM_RES_BITWORDS 76u        /* >= 16 x WM_PKT_MAXBYTES / 64: a word of 32 decided bits per trip of the wave */

struct K3ResArgs {
    K3Args k3;                   /* what k3_bursts ran with: the chip regions, the RSSI rows, and the packets, the byte arena and the counters it has just written */
    const float *dphi;           /* [2][S][Mcap] this push's soft symbols */
    const uint2 *src_pkts;       /* K3Args.lev_pkt: {the access-code chip's sample within the push, row} per packet slot */
    WmRescue *res_pkts;          /* [pkts_cap] pinned host memory: record i belongs to packet i */
};

/* Per-wave scratch: the decided bits (pair 32 t + k of the data = bit k of word t) and the telegram's bytes. */
struct K3ResLds { uint32_t bits[4][WM_RES_BITWORDS]; uint8_t bytes[4][WM_PKT_MAXBYTES + 4]; };

/* One packet record, by one wave. */
__device__ void rescue_item(const K3ResArgs &a, const uint32_t slot, const uint32_t ln, uint32_t *s_bits, uint8_t *s_bytes)
{
    const WmPush &g = a.k3.g;
    WmRescue rec = {};
    WmPkt p = a.k3.pkts[slot];
    const uint32_t L = p.L, n = 1u + 16u * L;                /* the chips the decoder would have taken, the access-code chip included */
    /* the subject, as far as the record says: an abort of the S1 chain's time2 decoder with a known length, at the chip behind a pair */
    const bool subject = p.status == WM_PKT_ABORT && p.algo == 1u && p.chain == 1u && L >= 12u && L <= WM_PKT_MAXBYTES && p.stream < g.S &&
                         (p.consumed & 1u) && p.consumed >= 19u && p.consumed <= n;
    if (!subject) { if (ln == 0) a.res_pkts[slot] = rec; return; }

    /* ---- the chips again, as k3_repair finds them: the access-code chip's segment from its sample, its index there from the counts ---- */
    K3Item it;
    it.algo = 1u; it.ch = 1u; it.stream = p.stream; it.cont = 0;
    it.nseg = g.nseg[1]; it.seg_len = g.seg_len[1];
    it.row = (uint64_t)g.S + it.stream;
    it.cnt = a.k3.counts[1] + it.row * g.nseg_cap[1];
    it.sidx0 = it.row * g.nseg_cap[1];
    const uint32_t rel = a.src_pkts[slot].x;                 /* the access-code chip's sample within the push */
    it.seg = min(rel / it.seg_len, it.nseg - 1u);
    uint32_t before = 0, total = 0;
    for (uint32_t s = ln; s < it.nseg; s += 64u) { const uint32_t c = it.cnt[s]; if (s < it.seg) before += c; total += c; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o); total += __shfl_xor(total, o); }
    /* all n chips lie inside the push's chip stream; anything else is not this kernel's to touch */
    if (p.chip0 < before || p.chip0 >= total || total - p.chip0 < n || rel >= g.M) { if (ln == 0) a.res_pkts[slot] = rec; return; }
    it.k = p.chip0 - before; it.chip0 = p.chip0; it.avail = total - p.chip0; it.n = n;
    const float *soft = a.dphi + it.row * g.Mcap;
    const uint8_t *rssi = a.k3.rssi + it.row * g.Mcap;

    /* ---- the data chips, 64 a trip: lane ln takes chip 1 + j0 + ln, so a pair sits on lanes 2 k and 2 k + 1 and never straddles a trip ---- */
    uint32_t first_bad = 0xFFFFFFFFu, stop = 0xFFFFFFFFu, margin = 0xFFFFFFFFu, pairs = 0, r_last = 0, pm_last = 0;
    for (uint32_t j0 = 0; j0 + 1u < n; j0 += 64u) {
        const uint32_t j = 1u + j0 + ln;
        uint32_t w = 0, pm = 0, rs = 255u;
        const bool in = j < n;
        if (in) {
            uint32_t sg, kk; k3_locate(it, j, sg, kk);
            w = k3_chip(a.k3, it, sg, kk);
            pm = sg * it.seg_len + WM_CHIP_POS(w);
            rs = pm < g.M ? rssi[pm] : 0u;
            /* a framer reset on a chip, the RSSI gate at a chip that does not complete the telegram: the reference would not have come through */
            if ((w & 4u) || (rs < 5u && j + 1u < n)) stop = min(stop, j);
        }
        const uint32_t v = w & 1u, vo = __shfl_xor(v, 1);
        const bool invalid = in && v == vo;
        if (invalid) first_bad = min(first_bad, (j0 + ln) >> 1);
        /* the soft symbols of the invalid pairs only; the larger one is the 1 */
        int32_t q = 0;
        if (invalid) q = pm < g.M ? lev_quant(soft[pm]) : 0;
        const int32_t qo = (int32_t)__shfl_xor((uint32_t)q, 1);
        uint32_t bit = 0;
        if (in && !(ln & 1u)) {                              /* the pair's first chip: q is q_a, qo is q_b */
            bit = invalid ? (qo > q) : vo;
            if (invalid) margin = min(margin, (uint32_t)(qo > q ? qo - q : q - qo));
        }
        pairs += (uint32_t)__popcll(__ballot(invalid && !(ln & 1u)));
        const uint32_t b2 = __shfl(bit, (int)((ln & 31u) * 2u));
        const uint32_t m = (uint32_t)__ballot(ln < 32u && b2);
        if (ln == 0) s_bits[j0 >> 6] = m;
        if (j + 1u == n) { r_last = rs; pm_last = pm; }
    }
    first_bad = rep_wave_min(first_bad); stop = rep_wave_min(stop); margin = rep_wave_min(margin);
    r_last = __shfl(r_last, (int)((n - 2u) & 63u)); pm_last = __shfl(pm_last, (int)((n - 2u) & 63u));
    WM_WAVE_SYNC();
    /* a Manchester violation and nothing else: the decoder stopped behind the FIRST invalid pair, no reset, no gate */
    if (stop != 0xFFFFFFFFu || first_bad == 0xFFFFFFFFu || p.consumed != 2u * first_bad + 3u) {
        if (ln == 0) a.res_pkts[slot] = rec;
        WM_WAVE_SYNC();
        return;
    }

    /* ---- bytes: lane b assembles byte b, b + 64, ...: pairs 8 b ... 8 b + 7, the first in the most significant bit ---- */
    for (uint32_t b = ln; b < L; b += 64u) s_bytes[b] = (uint8_t)(__brev((s_bits[b >> 2] >> (8u * (b & 3u))) & 255u) >> 24);
    WM_WAVE_SYNC();
    /* the frame-A block CRCs: lane i checks block i (12 bytes, then 18s, the last may be short), as burst_item does */
    uint32_t crc_bad = 0;
    {
        const uint32_t start = ln == 0 ? 0u : 12u + (ln - 1u) * 18u;
        if (start < L) {
            const uint32_t blk = min(ln == 0 ? 12u : 18u, L - start);
            crc_bad = blk < 2u || k3_crc16(s_bytes + start, blk - 2u) != (((uint32_t)s_bytes[start + blk - 2u] << 8) | s_bytes[start + blk - 1u]);
        }
    }
    crc_bad = __ballot(crc_bad) != 0ull;
    rec.pairs = (uint16_t)pairs; rec.min_margin = margin; rec.blocks = (uint16_t)(1u + (L - 12u + 17u) / 18u);
    rec.status = 2;
    if (!crc_bad) {
        /* all or nothing.  Storage first, as burst_item: a full arena is not asked again, and a telegram without room has no line */
        uint32_t boff = 0, ok = 0;
        if (ln == 0 && WM_PEEK(a.k3.n_bytes) <= a.k3.bytes_cap) {
            boff = atomicAdd(a.k3.n_bytes, (L + 3u) & ~3u);
            ok = boff <= a.k3.bytes_cap && a.k3.bytes_cap - boff >= L;
        }
        ok = __shfl(ok, 0); boff = __shfl(boff, 0);
        rec.status = ok ? 1 : 3;
        if (ok) {
            for (uint32_t b = ln; b < L; b += 64u) a.k3.bytes[boff + b] = s_bytes[b];
            if (ln == 0) {                                   /* status and consumed stay: the host's busy bookkeeping sees what it saw */
                p.flags = (uint8_t)(p.flags | WM_PKTF_CRC_OK | WM_PKTF_RESCUED);
                p.off = boff; p.sample = g.m0 + pm_last; p.rssi_now = (uint8_t)r_last;
                a.k3.pkts[slot] = p;
            }
        }
    }
    if (ln == 0) a.res_pkts[slot] = rec;
    WM_WAVE_SYNC();                                          /* the scratch is reused by the wave's next record */
}

/* Behind k3_bursts and the level stage, on the packet records: grid and priority as k3_repair and k3_quality, for the same reason.  A
 * wave returns from a record that is no subject after the 32-byte read of its header, and subjects are the exception. */
__global__ __launch_bounds__(256) void k3_rescue(K3ResArgs a)
{
    wm_framer_prio();
    __shared__ K3ResLds lds;
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t np = min(*a.k3.n_pkts, a.k3.pkts_cap);
    for (uint32_t r = blockIdx.x * 4u + wv; r < np; r += gridDim.x * 4u) rescue_item(a, r, ln, lds.bits[wv], lds.bytes[wv]);
}

#endif /* WM_K3_RESCUE_H */
