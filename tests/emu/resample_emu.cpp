/* resample_emu.cpp -- TEST INFRASTRUCTURE: k0_resample (device source wm_k0_resample.h) on the coroutine block emulator, driven
 * push by push the way wm_api.hip drives the kernel: the same launch arguments, the same double-buffered carried state. */
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

#include "wm_k0_resample.h"

namespace {
struct Emu {
    uint32_t L, M, T, tile, cur = 0, rem = 0;
    uint64_t n_in = 0, n_out = 0;
    std::vector<int16_t> taps;
    std::vector<uint32_t> hist[2];
    std::vector<uint8_t> rem_buf[2];
};
}

extern "C" {

void *wm_emu_k0_new(uint32_t L, uint32_t M, uint32_t T, const int16_t *taps, uint32_t tile)
{
    Emu *e = new Emu();
    e->L = L; e->M = M; e->T = T; e->tile = tile;
    e->taps.assign(taps, taps + (size_t)L * T);
    for (int i = 0; i < 2; i++) { e->hist[i].assign(T - 1u, 0u); e->rem_buf[i].assign(4096u, 128u); }
    return e;
}
void wm_emu_k0_free(void *p) { delete (Emu *)p; }
unsigned wm_emu_k0_pick_tile(uint32_t L, uint32_t M, uint32_t T) { return k0_pick_tile(L, M, T); }
unsigned wm_emu_k0_lds_bytes(uint32_t L, uint32_t M, uint32_t T, uint32_t tile) { return k0_lds_bytes(L, M, T, tile); }
unsigned wm_emu_k0_span(uint32_t L, uint32_t M, uint32_t T, uint32_t tile) { return k0_span(L, M, T, tile); }
/* A stream that is already in_first input samples and n_first outputs long (all of them x = 0, nothing waiting for a block): the next
 * push starts at these counters.  The host's k0_plan starts at 0 and has no such entry; only the kernel's 64-bit arguments are
 * reachable this way. */
void wm_emu_k0_start_at(void *p, uint64_t in_first, uint64_t n_first)
{
    Emu *e = (Emu *)p;
    e->n_in = in_first; e->n_out = n_first; e->rem = 0;
}

/* One push of raw_bytes (multiple of 4096) of one capture.  window: room for 4096 + 2 * outputs bytes; receives the remainder of
 * earlier pushes followed by this push's bytes.  Returns the bytes the pipeline would take (whole 4096-byte blocks). */
long wm_emu_k0_push(void *p, const uint8_t *raw, size_t raw_bytes, uint8_t *window, size_t window_cap)
{
    Emu *e = (Emu *)p;
    const uint32_t n_in = (uint32_t)(raw_bytes / 2u);
    const uint64_t out_end = ((e->n_in + n_in) * (uint64_t)e->L + e->M - 1u) / e->M;
    const uint32_t n_out = (uint32_t)(out_end - e->n_out);
    const size_t total = (size_t)e->rem + 2u * (size_t)n_out, whole = total / 4096u * 4096u;
    if (total > window_cap) return -1;
    K0Args a{};
    a.raw = raw; a.raw_stride = 0; a.out = window; a.out_stride = 0; a.taps = e->taps.data();
    a.hist_in = e->hist[e->cur].data(); a.hist_out = e->hist[e->cur ^ 1u].data();
    a.rem_in = e->rem_buf[e->cur].data(); a.rem_out = e->rem_buf[e->cur ^ 1u].data();
    a.n_first = e->n_out; a.in_first = e->n_in; a.n_in = n_in; a.n_out = n_out;
    a.rem_prev = e->rem; a.keep_from = (uint32_t)whole;
    a.L = e->L; a.M = e->M; a.T = e->T; a.tile = e->tile;
    std::vector<uint32_t> lds(k0_lds_bytes(e->L, e->M, e->T, e->tile) / 4u + 1u);
    gridDim = {(n_out + e->tile - 1u) / e->tile, 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) {
        blockIdx = {b, 0, 0};
        std::fill(lds.begin(), lds.end(), 0xDEADBEEFu);          /* what a block finds in LDS is not defined */
        block_emu::run_block(WM_K0_THREADS, [&] { k0_resample_block(a, lds.data()); });
    }
    e->n_in += n_in; e->n_out = out_end; e->rem = (uint32_t)(total - whole); e->cur ^= 1u;
    return (long)whole;
}

}
