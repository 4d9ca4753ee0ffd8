/* rescue_emu.cpp -- TEST INFRASTRUCTURE: k3_rescue (device source wm_k3_rescue.h) on the coroutine block emulator, driven the way
 * wm_api.hip's launch_k3 drives it: k3_scan and k3_bursts over settled chip regions (one capture, both chains, both framers) leave the
 * packets, the byte arena, its counter and every packet's access-code sample; k3_rescue then works on those, with this push's soft
 * symbols and RSSI bytes. */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "block_emu.h"

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static                  /* one block runs at a time: block-shared = static */
#define WM_WAVE_SYNC() emu_wave_barrier()
#define WM_PEEK(p) (*(p))
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
using std::max;
using std::min;
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
static inline int __popc(uint32_t v) { return __builtin_popcount(v); }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline uint32_t __brev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p += v; return o; }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }

#include "wm_dev.h"
#include "wm_k2_common.h"
#include "wm_k3_bursts.h"
#include "wm_k3_levels.h"
#include "wm_k3_repair.h"
#include "wm_k3_rescue.h"

extern "C" {

unsigned wm_emu_res_pkt_bytes(void) { return sizeof(WmPkt); }
unsigned wm_emu_res_record_bytes(void) { return sizeof(WmRescue); }
unsigned wm_emu_res_lds_bytes(void) { return sizeof(K3ResLds); }

/* geo: M, Mcap, flags, m0, seg_len[2], nseg[2], cap[2].  chips / counts / seen per framer [2][nseg][cap], [2][nseg]; rssi and dphi
 * [2][Mcap].  pkts_before receives the packets as k3_bursts left them, bytes_before the arena; pkts_out / bytes / recs_out what k3_rescue
 * made of them; counters: {the byte counter behind k3_bursts, behind k3_rescue, the packet counter behind k3_rescue}.  Returns the number
 * of packets, -1 if k3_bursts ran out of storage, -2 if k3_rescue wrote beyond the records or the arena it was given. */
long wm_emu_rescue(const uint64_t *geo, const uint32_t *chips0, const uint32_t *chips1, const uint32_t *counts0, const uint32_t *counts1,
                   const uint32_t *seen0, const uint32_t *seen1, const uint8_t *rssi, const float *dphi,
                   void *pkts_before, uint8_t *bytes_before, void *pkts_out, uint32_t pkts_cap, uint8_t *bytes, uint32_t bytes_cap, void *recs_out,
                   uint32_t *counters, uint32_t max_blocks)
{
    WmPush g{};
    g.S = 1; g.d = 2; g.M = (uint32_t)geo[0]; g.Mcap = (uint32_t)geo[1]; g.flags = (uint32_t)geo[2]; g.m0 = geo[3];
    for (int a = 0; a < 2; a++) {
        g.seg_len[a] = (uint32_t)geo[4 + a]; g.nseg[a] = (uint32_t)geo[6 + a]; g.nseg_cap[a] = g.nseg[a]; g.cap[a] = (uint32_t)geo[8 + a];
    }
    const uint32_t hits_cap = pkts_cap;
    std::vector<uint2> hits(hits_cap);
    uint32_t n_hits = 0, err = 0, n_hdr = 0, n_words = 0, n_pkts = 0, n_bytes = 0;
    gridDim = {(2u * (g.nseg[0] + g.nseg[1]) + 255u) / 256u, (std::max(g.cap[0], g.cap[1]) + WM_K3_SCAN_PART - 1u) / WM_K3_SCAN_PART, 1};
    for (uint32_t part = 0; part < gridDim.y; part++)
        for (uint32_t b = 0; b < gridDim.x; b++) {
            blockIdx = {b, part, 0};
            block_emu::run_block(256, [&] { k3_scan(g, chips0, chips1, counts0, counts1, seen0, seen1, hits.data(), &n_hits, hits_cap, &err); });
        }
    std::vector<WmBurstHdr> hdr(hits_cap + 4); std::vector<uint32_t> words(1u << 20);
    std::vector<WmPkt> pkts(pkts_cap + 2); std::vector<uint2> lev_pkt(pkts_cap + 2), lev_hdr(hits_cap + 4);
    /* the arena with a guard behind its capacity that nobody may touch */
    std::vector<uint8_t> arena((size_t)bytes_cap + 512, 0xC3);
    memset(arena.data(), 0, bytes_cap);
    const uint32_t pending[4] = {0, 0, 0, 0};
    K3Args k3{};
    k3.g = g; k3.rssi = rssi; k3.chips[0] = chips0; k3.chips[1] = chips1; k3.counts[0] = counts0; k3.counts[1] = counts1;
    k3.hits = hits.data(); k3.n_hits = &n_hits; k3.hits_cap = hits_cap; k3.pending = pending;
    k3.hdr = hdr.data(); k3.hdr_cap = hits_cap + 4; k3.words = words.data(); k3.words_cap = (uint32_t)words.size();
    k3.n_hdr = &n_hdr; k3.n_words = &n_words; k3.err = &err;
    k3.pkts = pkts.data(); k3.pkts_cap = pkts_cap; k3.bytes = arena.data(); k3.bytes_cap = bytes_cap; k3.n_pkts = &n_pkts; k3.n_bytes = &n_bytes;
    k3.lev_pkt = lev_pkt.data(); k3.lev_hdr = lev_hdr.data();
    gridDim = {std::max(1u, std::min((4u + std::min(n_hits, hits_cap) + 3u) / 4u, max_blocks)), 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, 0, 0}; block_emu::run_block(256, [&] { k3_bursts(k3, 0xFFFFFFFFu); }); }
    if (err || n_pkts > pkts_cap) return -1;
    memcpy(pkts_before, pkts.data(), n_pkts * sizeof(WmPkt));
    memcpy(bytes_before, arena.data(), bytes_cap);
    counters[0] = n_bytes;
    {
        /* two records of room beyond what was written, never to be touched; the counter says more than the capacity, as an overflowing push's does */
        const uint32_t np = n_pkts;
        WmRescue canary; memset(&canary, 0xA5, sizeof canary);
        std::vector<WmRescue> recs(np + 2, canary);
        WmPkt pc; memset(&pc, 0x5A, sizeof pc);
        pkts.resize(np + 2); pkts[np] = pc; pkts[np + 1] = pc;
        uint32_t counter = np + 2;
        K3ResArgs ra{};
        ra.k3 = k3; ra.k3.pkts = pkts.data(); ra.k3.pkts_cap = np; ra.k3.n_pkts = &counter;
        ra.dphi = dphi; ra.src_pkts = lev_pkt.data(); ra.res_pkts = recs.data();
        gridDim = {std::max(1u, std::min((np + 3u) / 4u, max_blocks)), 1, 1};
        for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, 0, 0}; block_emu::run_block(256, [&] { k3_rescue(ra); }); }
        for (uint32_t k = 0; k < 2; k++) if (memcmp(&recs[np + k], &canary, sizeof canary) || memcmp(&pkts[np + k], &pc, sizeof pc)) return -2;
        for (size_t k = bytes_cap; k < arena.size(); k++) if (arena[k] != 0xC3) return -2;
        memcpy(recs_out, recs.data(), np * sizeof(WmRescue));
        counters[1] = n_bytes; counters[2] = counter;
    }
    gridDim = {1, 1, 1}; blockIdx = {0, 0, 0};
    memcpy(bytes, arena.data(), bytes_cap);
    memcpy(pkts_out, pkts.data(), n_pkts * sizeof(WmPkt));
    return (long)n_pkts;
}

}
