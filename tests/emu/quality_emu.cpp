/* quality_emu.cpp -- TEST INFRASTRUCTURE: k3_quality (device source wm_k3_quality.h) on the coroutine block emulator, driven the way
 * wm_api.hip's launch_k3 drives it: k3_scan and k3_bursts over settled chip regions (one capture, both chains, both framers) leave the
 * packets, the byte arena and every packet's access-code sample; k3_quality then measures those on this push's soft symbols. */
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
static inline uint32_t __brev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p += v; return o; }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p |= v; return o; }

#include "wm_dev.h"
#include "wm_k2_common.h"
#include "wm_k3_bursts.h"
#include "wm_k3_levels.h"
#include "wm_k3_repair.h"
#include "wm_k3_quality.h"

extern "C" {

unsigned wm_emu_q_pkt_bytes(void) { return sizeof(WmPkt); }
unsigned wm_emu_q_record_bytes(void) { return sizeof(WmQuality); }

/* geo: M, Mcap, flags, m0, seg_len[2], nseg[2], cap[2].  chips / counts / seen per framer [2][nseg][cap], [2][nseg]; rssi and dphi
 * [2][Mcap].  pkts_before receives the packets as k3_bursts left them (with patch_slot < their number: that packet's L set to patch_L,
 * a length the burst kernel itself never writes), bytes_before the arena; pkts_out / bytes what they are behind k3_quality; recs_out
 * its records.  Returns the number of packets, -1 if k3_bursts ran out of storage, -2 if k3_quality wrote beyond the records it was
 * given. */
long wm_emu_quality(const uint64_t *geo, const uint32_t *chips0, const uint32_t *chips1, const uint32_t *counts0, const uint32_t *counts1,
                    const uint32_t *seen0, const uint32_t *seen1, const uint8_t *rssi, const float *dphi,
                    void *pkts_before, uint8_t *bytes_before, void *pkts_out, uint32_t pkts_cap, uint8_t *bytes, uint32_t bytes_cap, void *recs_out,
                    uint32_t max_blocks, uint32_t patch_slot, uint32_t patch_L)
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
    const uint32_t pending[4] = {0, 0, 0, 0};
    K3Args k3{};
    k3.g = g; k3.rssi = rssi; k3.chips[0] = chips0; k3.chips[1] = chips1; k3.counts[0] = counts0; k3.counts[1] = counts1;
    k3.hits = hits.data(); k3.n_hits = &n_hits; k3.hits_cap = hits_cap; k3.pending = pending;
    k3.hdr = hdr.data(); k3.hdr_cap = hits_cap + 4; k3.words = words.data(); k3.words_cap = (uint32_t)words.size();
    k3.n_hdr = &n_hdr; k3.n_words = &n_words; k3.err = &err;
    k3.pkts = pkts.data(); k3.pkts_cap = pkts_cap; k3.bytes = bytes; k3.bytes_cap = bytes_cap; k3.n_pkts = &n_pkts; k3.n_bytes = &n_bytes;
    k3.lev_pkt = lev_pkt.data(); k3.lev_hdr = lev_hdr.data();
    gridDim = {std::max(1u, std::min((4u + std::min(n_hits, hits_cap) + 3u) / 4u, max_blocks)), 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, 0, 0}; block_emu::run_block(256, [&] { k3_bursts(k3, 0xFFFFFFFFu); }); }
    if (err || n_pkts > pkts_cap) return -1;
    const uint32_t np = n_pkts;
    if (patch_slot < np) pkts[patch_slot].L = (uint16_t)patch_L;
    memcpy(pkts_before, pkts.data(), np * sizeof(WmPkt));
    memcpy(bytes_before, bytes, bytes_cap);
    {
        /* two records of room beyond what was written, never to be touched; the counter says more than the capacity, as an overflowing push's does */
        WmQuality canary; memset(&canary, 0xA5, sizeof canary);
        std::vector<WmQuality> recs(np + 2, canary);
        WmPkt pc; memset(&pc, 0x5A, sizeof pc);
        pkts.resize(np + 2); pkts[np] = pc; pkts[np + 1] = pc;
        uint32_t counter = np + 2;
        K3QualArgs qa{};
        qa.k3 = k3; qa.k3.pkts = pkts.data(); qa.k3.pkts_cap = np; qa.k3.n_pkts = &counter;
        qa.dphi = dphi; qa.src_pkts = lev_pkt.data(); qa.q_pkts = recs.data();
        gridDim = {std::max(1u, std::min((np + 3u) / 4u, max_blocks)), 1, 1};
        for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, 0, 0}; block_emu::run_block(256, [&] { k3_quality(qa); }); }
        for (uint32_t k = 0; k < 2; k++) if (memcmp(&recs[np + k], &canary, sizeof canary) || memcmp(&pkts[np + k], &pc, sizeof pc)) return -2;
        memcpy(recs_out, recs.data(), np * sizeof(WmQuality));
    }
    gridDim = {1, 1, 1}; blockIdx = {0, 0, 0};
    memcpy(pkts_out, pkts.data(), np * sizeof(WmPkt));
    return (long)np;
}

}
