/* level_emu.cpp -- TEST INFRASTRUCTURE: k3_levels and k3_level_tail (device source wm_k3_levels.h) on the coroutine block emulator, driven
 * push by push the way wm_api.hip's launch_k3 drives them: one capture, both chains, what k3_bursts would have left per record (the
 * access-code sample and the row of packets and of burst headers, continuations among them), the soft-symbol tail double-buffered
 * between pushes. */
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
using std::max;
using std::min;
struct uint2 { uint32_t x, y; };

#include "wm_dev.h"
#include "wm_k2_common.h"
#include "wm_k3_levels.h"

namespace {
struct Emu {
    std::vector<float> tail[2];                          /* [2 rows][WM_LEV_TAIL], guarded by 64 floats on either side */
    uint32_t cur = 0;
    uint64_t m0 = 0;
};
const float GUARD = 12345.0f;
}

extern "C" {

unsigned wm_emu_lev_record_bytes(void) { return sizeof(WmLevel); }
unsigned wm_emu_lev_tail(void) { return WM_LEV_TAIL; }

void *wm_emu_lev_new(void)
{
    Emu *e = new Emu();
    for (auto &t : e->tail) { t.assign(64 + 2 * WM_LEV_TAIL + 64, GUARD); std::fill(t.begin() + 64, t.end() - 64, 0.0f); }      /* as wmbus_open zeroes it */
    return e;
}
void wm_emu_lev_free(void *p) { delete (Emu *)p; }

/* One push of M decimated samples: dphi [2][Mcap] (row = chain), n items {rel: access-code sample within the push, chain, kind: 0 / 1 a packet
 * (of either framer), 2 a burst header, 3 a continuation header}.  out[i] receives item i's record.  Returns 0, or a
 * negative number if the kernels wrote outside their arrays. */
long wm_emu_lev_push(void *p, const float *dphi, uint32_t M, uint32_t Mcap, const uint32_t *rel, const uint8_t *chain, const uint8_t *kind, uint32_t n, void *out)
{
    Emu *e = (Emu *)p;
    WmPush g{};
    g.S = 1; g.d = 2; g.M = M; g.Mcap = Mcap; g.m0 = e->m0;
    /* what k3_bursts leaves per slot: {access-code sample within the push (~0: a continuation), row}; packets and headers in item order */
    std::vector<uint2> sp, sh;
    std::vector<uint32_t> slot(n);
    for (uint32_t i = 0; i < n; i++) {
        std::vector<uint2> &v = kind[i] < 2 ? sp : sh;
        slot[i] = (uint32_t)v.size();
        v.push_back(uint2{kind[i] == 3 ? 0xFFFFFFFFu : rel[i], chain[i]});
    }
    /* two records of room beyond what was written, never to be touched; the counters say more than the capacity, as an overflowing push's do */
    const uint32_t np = (uint32_t)sp.size(), nh = (uint32_t)sh.size();
    WmLevel canary; memset(&canary, 0xA5, sizeof canary);
    std::vector<WmLevel> lp(np + 2, canary), lh(nh + 2, canary);
    sp.resize(np + 2, uint2{0u, 0u}); sh.resize(nh + 2, uint2{0u, 0u});
    uint32_t n_pkts = np + 2, n_hdr = nh + 2;
    K3LevArgs a{};
    a.g = g; a.dphi = dphi;
    a.tail_in = e->tail[e->cur].data() + 64; a.tail_out = e->tail[e->cur ^ 1u].data() + 64;
    a.src_pkts = sp.data(); a.n_pkts = &n_pkts; a.pkts_cap = np;
    a.src_hdr = sh.data(); a.n_hdr = &n_hdr; a.hdr_cap = nh;
    a.lev_pkts = lp.data(); a.lev_hdr = lh.data();
    gridDim = {3, 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, 0, 0}; block_emu::run_block(256, [&] { k3_levels(a); }); }
    gridDim = {(WM_LEV_TAIL + 255u) / 256u, 2, 1};
    for (uint32_t y = 0; y < 2; y++)
        for (uint32_t b = 0; b < gridDim.x; b++) { blockIdx = {b, y, 0}; block_emu::run_block(256, [&] { k3_level_tail(a); }); }
    gridDim = {1, 1, 1}; blockIdx = {0, 0, 0};
    for (uint32_t k = 0; k < 2; k++) if (memcmp(&lp[np + k], &canary, sizeof canary) || memcmp(&lh[nh + k], &canary, sizeof canary)) return -1;
    for (auto &t : e->tail) for (uint32_t k = 0; k < 64; k++) if (t[k] != GUARD || t[t.size() - 1 - k] != GUARD) return -2;
    for (uint32_t i = 0; i < n; i++) ((WmLevel *)out)[i] = kind[i] < 2 ? lp[slot[i]] : lh[slot[i]];
    e->cur ^= 1u; e->m0 += M;
    return 0;
}

/* the tail the next push will read, row by row */
void wm_emu_lev_read_tail(void *p, float *dst) { Emu *e = (Emu *)p; memcpy(dst, e->tail[e->cur].data() + 64, 2u * WM_LEV_TAIL * sizeof(float)); }

}
