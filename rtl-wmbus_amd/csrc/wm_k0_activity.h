/*
 * wm_k0_activity.h -- K0 channel activity: one record per burst of energy in every pipeline row's channel, decoded or not
 * (cfg.channel_activity).
 *
 * k0_channel_power (wm_k0_power.h) leaves P[r][K], the power in row r's 200 kHz channel in level block K.  k0_activity, launched behind
 * it, turns every row's timeline into a census: epochs of 64 level blocks, the lower quartile of each, a floor that is the smallest
 * quartile of the last H + 1 epochs, a block active where it lies T / 256 above that floor, and a record per maximal run of at least two
 * active blocks.  The arithmetic is the definition (include/wmbus_hip.h, CHANNEL ACTIVITY; tests/activity_ref.py restates it): integers
 * only, every division floors.
 *
 * Shape: one wave per pipeline row, a lane is a level block of the epoch, the wave walks the row's complete epochs of this push in order
 * -- the up to 63 blocks the last push left over first.  Per epoch, all of it wave-level:
 *   quartile   a lane's rank = how many of the 64 values are smaller, or equal and in a lower lane: 64 broadcasts of one lane's value
 *              (v_readlane: the index is the loop's, a scalar, and the comparison reads a scalar; no LDS, no sort network), and
 *              the lane of rank 16 holds the quartile
 *   floor      lane j keeps the quartile of the j-th epoch back (j < H; 2^32 - 1 beyond and before the stream), the floor is a six-step
 *              xor minimum over the ring and the new quartile, and the ring moves up one lane
 *   mask       m = __ballot(P x 256 > T x floor); starts m & ~(m << 1 | open), ends ~m & (m << 1 | open): bit operations on a mask every
 *              lane holds
 *   run sums   a segmented inclusive prefix sum in 64 bits, six steps: lane i takes lane i - d's sum where no segment starts in
 *              (i - d, i] -- read off the mask, so only the sums travel.  The lane behind a run's last block closes it
 *   records    a run of >= 2 blocks is a record; the closing lanes of an epoch take consecutive tickets of an arena (one atomic of lane 0
 *              per epoch that closes any; the counter is never reset, the host names its value in front of the push) and write their
 *              records with plain vector stores.  The host sorts by (row, first_block): the order of the tickets does not reach the caller
 * The exchanges are __shfl / __shfl_xor (ds_bpermute_b32: any lane distance, 64 lanes) rather than DPP: a prefix step reaches 32 lanes back
 * and the ring shift crosses the rows of 16 lanes that DPP's row controls stay inside; the wave-wide DPP shifts are not gfx9's to rely on.
 * One wave per row is latency bound whatever it uses -- an epoch is about 200 instructions -- and rows run side by side.
 *
 * The row's carried state stays on the device and advances exactly once per push (wm_api.hip launches this kernel where pw.K moves on):
 * the values of the incomplete epoch, the ring, the epoch count and the open run.  The stream's last incomplete epoch is never evaluated.
 *
 * The rest of the file is host code shared with the library's entry points: the rule over a whole timeline, and the matching.
 */
#ifndef WM_K0_ACTIVITY_H
#define WM_K0_ACTIVITY_H

#include <algorithm>
#include <vector>

#include "wm_k0_power.h"

#define WM_K0_ACT_EPOCH_LOG2  6u          /* an epoch: 64 level blocks, a lane each */
#define WM_K0_ACT_QUARTILE    16u         /* the element at this index of an epoch's ascending P */
#define WM_K0_ACT_RATIO_Q8    1024u       /* cfg.channel_activity_ratio_q8 = 0 */
#define WM_K0_ACT_NONE        0xFFFFFFFFu /* a ring entry no epoch has filled */

/* H = min(63, ceil(0.16 Fin / 32768) + 1) epochs behind the current one: 0.16 s is longer than the longest telegram */
__host__ __device__ __forceinline__ uint32_t k0_act_epochs(uint32_t in_hz)
{
    const uint32_t h = (uint32_t)(((uint64_t)in_hz + 204799u) / 204800u) + 1u;
    return h > 63u ? 63u : h;
}
/* the records one row can close in one push of n_blk level blocks: a record takes two active blocks and the inactive one behind them, the
 * 63 blocks carried in count, and a run carried in needs only its closing block here */
__host__ __device__ __forceinline__ uint32_t k0_act_row_cap(uint32_t n_blk) { return (n_blk + 63u) / 3u + 2u; }

struct K0ActState {                       /* one pipeline row */
    uint32_t tail[64];                    /* P of the incomplete epoch, n_tail of them */
    uint32_t ring[64];                    /* [j] the quartile of the j-th epoch back, j < H; WM_K0_ACT_NONE otherwise */
    uint64_t epochs;                      /* complete epochs so far: the next epoch's first level block is epochs << 6 */
    uint64_t run_first, run_sum;          /* the open run: its first level block, the sum of its P so far */
    uint32_t run_blocks, run_floor;       /* run_blocks = 0: no run is open */
    uint32_t n_tail, pad;
};
struct K0ActRecord { uint64_t first_block; uint32_t blocks, mean, floor, row; };

struct K0ActArgs {
    const uint32_t *P;                    /* [rows][p_stride] K0PowArgs.P of this push */
    uint32_t p_stride, n_blk, rows;
    uint32_t T, H;                        /* the threshold in Q8 (257 ... 65535), the floor's epochs behind the current one */
    K0ActState *st;                       /* [rows] read and written: the state advances with every launch */
    K0ActRecord *arena;                   /* [cap] this push's records in ticket order */
    uint32_t *count;                      /* the tickets taken since the context opened; never reset, wraps */
    uint32_t base, cap;                   /* *count in front of this launch: ticket t lies at arena[t - base]; the arena's records */
};

/* v of lane `src`, src the same in every lane: a broadcast.  On the device this is v_readlane_b32. */
__device__ __forceinline__ uint32_t k0_act_bcast(uint32_t v, uint32_t src)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
#else
    return __shfl(v, (int)src);
#endif
}
__device__ __forceinline__ uint64_t k0_act_from(uint64_t v, uint32_t src)          /* v of lane src (any src < 64 per lane) */
{
    const uint32_t lo = __shfl((uint32_t)v, (int)src), hi = __shfl((uint32_t)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

/* One wave: blockIdx.x = pipeline row.  Every lane takes part in every exchange; all branches around exchanges are wave-uniform. */
__device__ __forceinline__ void k0_activity_wave(const K0ActArgs &a)
{
    const uint32_t row = blockIdx.x, lane = threadIdx.x & 63u;
    if (row >= a.rows) return;
    K0ActState &st = a.st[row];
    const uint32_t *P = a.P + (uint64_t)row * a.p_stride;
    const uint32_t n_tail = st.n_tail & 63u, total = n_tail + a.n_blk, n_ep = total >> WM_K0_ACT_EPOCH_LOG2;
    uint32_t ring = st.ring[lane];
    uint64_t epochs = st.epochs, run_first = st.run_first, run_sum = st.run_sum;
    uint32_t run_blocks = st.run_blocks, run_floor = st.run_floor;
    const uint64_t below = (1ull << lane) - 1ull;                /* the lanes under this one */
    WM_K0_WAVE_SYNC();                                           /* every lane has read the state before lane 0 writes the next */

    for (uint32_t ep = 0; ep < n_ep; ep++) {
        const uint32_t idx = (ep << WM_K0_ACT_EPOCH_LOG2) + lane;              /* < total: idx - n_tail < n_blk */
        const uint32_t p = idx < n_tail ? st.tail[idx] : P[idx - n_tail];
        /* the lower quartile: the value of rank 16 in the order (value, lane) */
        uint32_t rank = 0u;
#pragma unroll 8
        for (uint32_t j = 0; j < 64u; j++) {                                   /* eight broadcasts in flight: all 64 at once spill scalar registers */
            const uint32_t o = k0_act_bcast(p, j);
            rank += (o < p || (o == p && j < lane)) ? 1u : 0u;
        }
        const uint64_t at = __ballot(rank == WM_K0_ACT_QUARTILE);             /* exactly one lane: the ranks are a permutation */
        const uint32_t q = __shfl(p, (int)(__ffsll((long long)at) - 1));
        /* the floor: the smallest of q and the ring */
        uint32_t fl = ring < q ? ring : q;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(fl, m); fl = o < fl ? o : fl; }
        const uint32_t up = __shfl(ring, (int)((lane + 63u) & 63u));
        ring = lane == 0u ? q : lane < a.H ? up : WM_K0_ACT_NONE;
        /* the mask, the edges of the runs */
        const uint64_t m = __ballot((uint64_t)p * 256u > (uint64_t)a.T * fl);
        const uint64_t prev = (m << 1) | (run_blocks ? 1ull : 0ull);           /* bit i: block i - 1 is active */
        const uint64_t starts = m & ~prev, ends = ~m & prev;
        const uint64_t bounds = starts | ~m;                                  /* an inactive block is a segment of its own, sum 0 */
        /* the segmented inclusive sum: lane i takes lane i - d's where no segment begins in (i - d, i] */
        uint64_t sum = (m >> lane & 1ull) ? (uint64_t)p : 0ull;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t o = k0_act_from(sum, (lane + 64u - d) & 63u);
            const uint64_t span = lane >= d ? (bounds >> (lane - d + 1u)) & ((1ull << d) - 1ull) : 1ull;
            sum += span ? 0ull : o;
        }
        const uint64_t before = k0_act_from(sum, (lane + 63u) & 63u);          /* the sum of the run that ends in lane - 1 */
        /* the lane behind a run's last block closes it */
        const uint64_t k0 = epochs << WM_K0_ACT_EPOCH_LOG2;
        const uint64_t mine = starts & below;                                 /* the starts under this lane: the highest is this run's */
        K0ActRecord rec{};
        if (mine) {
            const uint32_t s = 63u - (uint32_t)__clzll((long long)mine);
            rec.first_block = k0 + s; rec.blocks = lane - s; rec.floor = fl;
            rec.mean = rec.blocks ? (uint32_t)(before / rec.blocks) : 0u;
        } else {                                                              /* the run came in open */
            const uint64_t all = run_sum + (lane ? before : 0ull);
            rec.first_block = run_first; rec.blocks = run_blocks + lane; rec.floor = run_floor;
            rec.mean = rec.blocks ? (uint32_t)(all / rec.blocks) : 0u;
        }
        rec.row = row;
        const bool closes = (ends >> lane & 1ull) && rec.blocks >= 2u;
        const uint64_t closing = __ballot(closes);
        if (closing) {                                                        /* the same in every lane */
            uint32_t base = 0u;
            if (lane == 0u) base = atomicAdd(a.count, (uint32_t)__popcll(closing));
            base = __shfl(base, 0);
            const uint32_t slot = base - a.base + (uint32_t)__popcll(closing & below);
            if (closes && slot < a.cap) a.arena[slot] = rec;
        }
        /* what stays open behind the epoch */
        const uint64_t last = k0_act_from(sum, 63u);
        if (m >> 63) {
            if (starts) {
                const uint32_t s = 63u - (uint32_t)__clzll((long long)starts);
                run_first = k0 + s; run_blocks = 64u - s; run_sum = last; run_floor = fl;
            } else { run_blocks += 64u; run_sum += last; }                    /* all 64 active behind an open run */
        } else run_blocks = 0u;
        epochs++;
    }
    /* the incomplete epoch: a lane reads its value before it writes the same slot */
    const uint32_t rem = total & 63u, idx = (n_ep << WM_K0_ACT_EPOCH_LOG2) + lane;
    if (lane < rem) st.tail[lane] = idx < n_tail ? st.tail[idx] : P[idx - n_tail];
    st.ring[lane] = ring;
    if (lane == 0u) {
        st.epochs = epochs; st.run_first = run_first; st.run_sum = run_sum; st.run_blocks = run_blocks; st.run_floor = run_floor;
        st.n_tail = rem;
    }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64) k0_activity(K0ActArgs a) { k0_activity_wave(a); }
#endif

/* ---- host: the rule over a whole timeline, and the matching ------------------------------------------------------------------------- */

struct K0ActBurst { uint64_t first_block; uint32_t blocks, mean, floor; };

/* p[0 .. n) = P of level blocks 0 .. n - 1 of one row; T = 257 ... 65535.  Plain loops, written apart from the kernel. */
static inline void k0_activity_rule(const uint32_t *p, size_t n, uint32_t in_hz, uint32_t T, std::vector<K0ActBurst> &out)
{
    const size_t n_ep = n >> WM_K0_ACT_EPOCH_LOG2, H = k0_act_epochs(in_hz);
    std::vector<uint32_t> q(n_ep), fl(n_ep), sorted(64u);
    for (size_t e = 0; e < n_ep; e++) {
        std::copy(p + 64u * e, p + 64u * e + 64u, sorted.begin());
        std::sort(sorted.begin(), sorted.end());
        q[e] = sorted[WM_K0_ACT_QUARTILE];
        fl[e] = *std::min_element(q.begin() + (e > H ? e - H : 0u), q.begin() + e + 1u);
    }
    uint64_t first = 0, sum = 0; uint32_t blocks = 0;
    for (size_t K = 0; K < 64u * n_ep; K++) {
        const bool act = (uint64_t)p[K] * 256u > (uint64_t)T * fl[K >> WM_K0_ACT_EPOCH_LOG2];
        if (act) { if (!blocks) { first = K; sum = 0; } blocks++; sum += p[K]; }
        else {
            if (blocks >= 2u) out.push_back(K0ActBurst{first, blocks, (uint32_t)(sum / blocks), fl[first >> WM_K0_ACT_EPOCH_LOG2]});
            blocks = 0;
        }
    }
}

/* a line whose access code lies in level block ka matches the burst with first_block - 1 <= ka < first_block + blocks */
static inline bool k0_activity_matches(uint64_t first_block, uint32_t blocks, uint64_t ka)
{
    return ka + 1u >= first_block && ka < first_block + blocks;
}

#endif
