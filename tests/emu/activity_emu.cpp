/* activity_emu.cpp -- TEST INFRASTRUCTURE: channel activity (cfg.channel_activity) on the coroutine block emulator.
 *   wm_emu_act_*   the device source of k0_activity (wm_k0_activity.h: k0_activity_wave) on the grid wm_api.hip launches -- a wave per
 *                  pipeline row -- driven push by push the way wm_api.hip drives it: the rows' state stays in the emulator between the
 *                  pushes, the ticket counter is never reset, and a push's records come back sorted by (row, first_block) as wait_gpu
 *                  sorts them.
 * The wave shims the kernel needs beyond block_emu.h live here: bit counts, and the atomic of the one lane that takes an epoch's tickets
 * (the emulator runs one coroutine at a time).  The twin of power_emu.cpp. */
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "block_emu.h"

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define WM_K0_WAVE_SYNC() emu_wave_barrier()

static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p = old + v; return old; }

#include "wm_k0_activity.h"

namespace {
struct Emu {
    uint32_t rows, in_hz, T;
    uint32_t count;
    std::vector<K0ActState> st;
};
}

extern "C" {

/* count0: what the ticket counter holds when the stream begins (the tickets wrap: a test starts close to 2^32) */
void *wm_emu_act_new(uint32_t rows, uint32_t in_hz, uint32_t ratio_q8, uint32_t count0)
{
    Emu *e = new Emu();
    e->rows = rows; e->in_hz = in_hz; e->T = ratio_q8 ? ratio_q8 : WM_K0_ACT_RATIO_Q8; e->count = count0;
    e->st.assign(rows, K0ActState{});
    for (K0ActState &s : e->st) std::fill(s.ring, s.ring + 64, WM_K0_ACT_NONE);
    return e;
}
void wm_emu_act_free(void *p) { delete (Emu *)p; }

/* One push: P = [rows][n_blk].  out receives {first_block, blocks, mean, floor, row} as five uint64 per record, at most cap records;
 * returns the records of the push, or -1 where the kernel took more tickets than k0_act_row_cap allows. */
long wm_emu_act_push(void *p, const uint32_t *P, uint32_t n_blk, uint64_t *out, size_t cap)
{
    Emu *e = (Emu *)p;
    if (!n_blk) return 0;
    const uint32_t arena_cap = e->rows * k0_act_row_cap(n_blk);
    std::vector<K0ActRecord> arena(arena_cap, K0ActRecord{0xDEADBEEFDEADBEEFull, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu});
    K0ActArgs a{};
    a.P = P; a.p_stride = n_blk; a.n_blk = n_blk; a.rows = e->rows; a.T = e->T; a.H = k0_act_epochs(e->in_hz);
    a.st = e->st.data(); a.arena = arena.data(); a.count = &e->count; a.base = e->count; a.cap = arena_cap;
    gridDim = {e->rows, 1, 1};
    for (uint32_t r = 0; r < e->rows; r++) {
        blockIdx = {r, 0, 0};
        block_emu::run_block(64u, [&] { k0_activity_wave(a); });
    }
    blockIdx = {0, 0, 0};
    const uint32_t n = e->count - a.base;
    if (n > arena_cap) return -1;
    std::sort(arena.begin(), arena.begin() + n, [](const K0ActRecord &x, const K0ActRecord &y) { return x.row != y.row ? x.row < y.row : x.first_block < y.first_block; });
    for (uint32_t i = 0; i < n && i < cap; i++) {
        out[5 * i] = arena[i].first_block; out[5 * i + 1] = arena[i].blocks; out[5 * i + 2] = arena[i].mean; out[5 * i + 3] = arena[i].floor; out[5 * i + 4] = arena[i].row;
    }
    return (long)n;
}

/* {n_tail, epochs, run_blocks} of a row: what the tests look at between pushes */
void wm_emu_act_state(void *p, uint32_t row, uint64_t *out)
{
    const K0ActState &s = ((Emu *)p)->st[row];
    out[0] = s.n_tail; out[1] = s.epochs; out[2] = s.run_blocks;
}

uint32_t wm_emu_act_epochs(uint32_t in_hz) { return k0_act_epochs(in_hz); }
uint32_t wm_emu_act_row_cap(uint32_t n_blk) { return k0_act_row_cap(n_blk); }

}
