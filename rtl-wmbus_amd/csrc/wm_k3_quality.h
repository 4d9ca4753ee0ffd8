/* wm_k3_quality.h -- cfg.line_quality: the chip rate, the jitter of the decision instants and the eye of the soft symbols of every time2
 * telegram that k3_bursts has decoded whole inside the push (the rule: include/wmbus_hip.h, LINE QUALITY; tests/quality_ref.py restates
 * it).  Device code, included by wm_kernels.hip behind wm_k3_repair.h: it runs behind k3_bursts and the level stage and reads what
 * k3_repair reads -- chip regions, counts, soft symbols, packet headers -- and writes nothing but its own records, so its place before or
 * behind k3_repair does not matter (a repair flips chips in its LDS copy, never in the chip regions). */
#ifndef WM_K3_QUALITY_H
#define WM_K3_QUALITY_H

typedef wmbus_quality WmQuality;   /* the kernel writes the very records wmbus_line_quality() hands out */

struct K3QualArgs {
    K3Args k3;                   /* what k3_bursts ran with: the chip regions and the packets it has just written */
    const float *dphi;           /* [2][S][Mcap] this push's soft symbols */
    const uint2 *src_pkts;       /* K3Args.lev_pkt: {the access-code chip's sample within the push, row} per packet slot */
    WmQuality *q_pkts;           /* [pkts_cap] pinned host memory: record i belongs to packet i */
};

__device__ __forceinline__ int64_t qual_wave_sum(int64_t v)
{
    uint32_t lo = (uint32_t)(uint64_t)v, hi = (uint32_t)((uint64_t)v >> 32);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
        const uint64_t s = (((uint64_t)hi << 32) | lo) + (((uint64_t)oh << 32) | ol);
        lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
    }
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int32_t qual_wave_min(int32_t v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const int32_t o = (int32_t)__shfl_xor((uint32_t)v, off); v = o < v ? o : v; }
    return v;
}

/* A lane's walk over its chips ln, ln + 64, ...: (sg, kk) of the chip 64 further on, from the one it stands on. */
__device__ __forceinline__ void qual_next(const K3Item &it, uint32_t &sg, uint32_t &kk)
{
    kk += 64u;
    while (sg < it.nseg) { const uint32_t c = it.cnt[sg]; if (kk < c) break; kk -= c; sg++; }
}

__device__ __forceinline__ int64_t qual_hz(int64_t x, int64_t N) { return lev_floordiv(3125 * x + 4096 * N, 8192 * N); }

/* One packet record, by one wave.  No LDS: the second pass (e, spread, the smallest margin need A, B, m1, m0 of the first) walks the
 * chips again -- 4673 chips of (p, q, v) per wave would be 37 KB, 150 KB a block, and would take the demodulation kernel's blocks off
 * the CU (the occupancy note at k3_repair); the chip words and soft symbols of the second walk come from the cache the first filled. */
__device__ void quality_item(const K3QualArgs &a, const uint32_t slot, const uint32_t ln)
{
    const WmPush &g = a.k3.g;
    WmQuality rec = {};
    const WmPkt p = a.k3.pkts[slot];
    const bool subject = p.status == WM_PKT_DONE && p.algo == 1u && p.L <= WM_PKT_MAXBYTES && p.stream < g.S && p.chain < 2u;
    if (!subject) { if (ln == 0) a.q_pkts[slot] = rec; return; }
    const uint32_t mode = p.chain ? 2u : (p.flags & WM_PKTF_C1) ? 1u : 0u;
    const uint32_t cpb = mode == 0u ? 12u : mode == 1u ? 8u : 16u, off = mode == 1u ? 17u : 1u;
    const uint32_t n = off + cpb * p.L;                      /* <= 1 + 16 x 292 = 4673 */

    /* ---- the chips again, as k3_repair finds them: the access-code chip's segment from its sample, its index from the counts ---- */
    K3Item it;
    it.algo = 1u; it.ch = p.chain; it.stream = p.stream; it.cont = 0;
    it.nseg = g.nseg[1]; it.seg_len = g.seg_len[1];
    it.row = (uint64_t)it.ch * g.S + it.stream;
    it.cnt = a.k3.counts[1] + it.row * g.nseg_cap[1];
    it.sidx0 = it.row * g.nseg_cap[1];
    const uint32_t rel = a.src_pkts[slot].x;
    it.seg = min(rel / it.seg_len, it.nseg - 1u);
    uint32_t before = 0, total = 0;
    for (uint32_t s = ln; s < it.nseg; s += 64u) { const uint32_t c = it.cnt[s]; if (s < it.seg) before += c; total += c; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o); total += __shfl_xor(total, o); }
    if (n < 2u || p.chip0 < before || p.chip0 >= total || total - p.chip0 < n || rel >= g.M) { if (ln == 0) a.q_pkts[slot] = rec; return; }
    it.k = p.chip0 - before; it.chip0 = p.chip0; it.avail = total - p.chip0; it.n = n;
    const float *row = a.dphi + it.row * g.Mcap;

    uint32_t sg0, kk0;
    k3_locate(it, 0u, sg0, kk0);
    const int64_t pos0 = (int64_t)(sg0 * it.seg_len + WM_CHIP_POS(k3_chip(a.k3, it, sg0, kk0)));
    uint32_t sgl, kkl;
    k3_locate(it, ln, sgl, kkl);                             /* this lane's first chip (it may lie beyond n: then it is never read) */

    /* ---- first pass: sum p, sum j' p, S1, S0, n1, and p[n-1] ---- */
    int64_t sp = 0, num = 0, S1 = 0, S0 = 0, plast = 0;
    uint32_t n1 = 0;
    {
        uint32_t sg = sgl, kk = kkl;
        for (uint32_t j = ln; j < n; j += 64u) {
            const uint32_t w = k3_chip(a.k3, it, sg, kk), pm = sg * it.seg_len + WM_CHIP_POS(w);
            const int64_t pj = (int64_t)pm - pos0;
            const int32_t q = pm < g.M ? lev_quant(row[pm]) : 0;
            sp += pj; num += (2 * (int64_t)j - (int64_t)(n - 1u)) * pj;
            if (w & 1u) { S1 += q; n1++; } else S0 += q;
            if (j == n - 1u) plast = pj;
            qual_next(it, sg, kk);
        }
    }
    sp = qual_wave_sum(sp); num = qual_wave_sum(num); S1 = qual_wave_sum(S1); S0 = qual_wave_sum(S0); plast = qual_wave_sum(plast);
    n1 = (uint32_t)lev_wave_sum((int32_t)n1);
    const uint32_t n0 = n - n1;
    if (plast >= (1 << 17) || num <= 0 || n1 == 0u || n0 == 0u) { if (ln == 0) a.q_pkts[slot] = rec; return; }

    const int64_t N = (int64_t)n, den = N * (N * N - 1) / 3;
    const int64_t B = lev_floordiv(4 * 65536 * num + den, 2 * den);
    const int64_t s = 65536 * sp - B * (N * (N - 1) / 2);
    const int64_t A = lev_floordiv(2 * s + N, 2 * N);
    const int64_t m1 = lev_floordiv(2 * S1 + (int64_t)n1, 2 * (int64_t)n1), m0 = lev_floordiv(2 * S0 + (int64_t)n0, 2 * (int64_t)n0);
    const int64_t mid = lev_floordiv(m1 + m0, 2);
    const bool up = m1 >= m0;

    /* ---- second pass: e, spread, the smallest margin ---- */
    int64_t e = 0, spread = 0;
    int32_t eye = 0x7FFFFFFF;
    {
        uint32_t sg = sgl, kk = kkl;
        for (uint32_t j = ln; j < n; j += 64u) {
            const uint32_t w = k3_chip(a.k3, it, sg, kk), pm = sg * it.seg_len + WM_CHIP_POS(w);
            const int64_t pj = (int64_t)pm - pos0;
            const int64_t q = pm < g.M ? lev_quant(row[pm]) : 0;
            const int64_t d = 65536 * pj - B * (int64_t)j - A;
            e += d >= 0 ? d : -d;
            const int64_t dq = q - ((w & 1u) ? m1 : m0);
            spread += dq >= 0 ? dq : -dq;
            const int64_t mg = ((w & 1u) != 0u) == up ? q - mid : mid - q;      /* sigma (q - mid) for a 1, sigma (mid - q) for a 0 */
            eye = min(eye, (int32_t)mg);
            qual_next(it, sg, kk);
        }
    }
    e = qual_wave_sum(e); spread = qual_wave_sum(spread); eye = qual_wave_min(eye);

    rec.n = n;
    rec.chip_rate_chz = (uint32_t)lev_floordiv(80000000ll * den + num, 2 * num);
    rec.jitter_ns = (uint32_t)lev_floordiv(1250 * e + 32768 * N, 65536 * N);
    rec.hi_hz = (int32_t)qual_hz(m1, 1); rec.lo_hz = (int32_t)qual_hz(m0, 1);
    rec.spread_hz = (uint32_t)qual_hz(spread, N);
    rec.eye_hz = (int32_t)qual_hz(eye, 1);
    if (ln == 0) a.q_pkts[slot] = rec;
}

/* Behind k3_bursts and the level stage, on the packet records: grid and priority as k3_repair, for the same reason.  A wave returns
 * from a record that is no subject after the 32-byte read of its header. */
__global__ __launch_bounds__(256) void k3_quality(K3QualArgs a)
{
    wm_framer_prio();
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t np = min(*a.k3.n_pkts, a.k3.pkts_cap);
    for (uint32_t r = blockIdx.x * 4u + wv; r < np; r += gridDim.x * 4u) quality_item(a, r, ln);
}

#endif /* WM_K3_QUALITY_H */
