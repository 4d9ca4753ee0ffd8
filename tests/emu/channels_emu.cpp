/* channels_emu.cpp -- TEST INFRASTRUCTURE: the channels form of K0 (device source wm_k0_resample.h: k0_resample_block_t<FMT, true, false,
 * false, true> and k0_convert_block<FMT, true, false, false, true>, what k0_resample_ch<> and k0_convert_ch<> run, behind k0_dc_sums /
 * k0_dc_plan / k0_agc_gain where the blocker or the AGC is on) on the coroutine block emulator, driven push by push the way wm_api.hip
 * drives the kernels: n_cap captures side by side, n_ch channels each, the grid's y the pipeline stream v = capture * n_ch + channel, the
 * raw bytes and the level tables one row per CAPTURE, history, remainder and window one row per PIPELINE STREAM, the same double-buffered
 * carried state, one clip counter for the whole push.  The twin of shift_emu.cpp / dc_emu.cpp / agc_emu.cpp. */
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
    uint32_t fmt, gain, L, M, T, tile, n_cap, n_ch, S, R, agc, blk_stride, cur = 0, rem = 0, last_blk = 0;
    uint32_t steps[WM_K0_MAX_CH];
    bool resample;
    uint64_t n_in = 0, n_out = 0;
    std::vector<int16_t> taps;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    std::vector<uint32_t> hist[2];                               /* [S][T - 1] */
    std::vector<uint8_t> rem_buf[2];                             /* [S][4096] */
    std::vector<K0DcState> st[2];                                /* [n_cap] */
    std::vector<K0S2> sums;                                      /* [n_cap][blk_stride] */
    std::vector<uint32_t> dc_tab;                                /* [n_cap][blk_stride] */
    std::vector<uint16_t> agc_tab;                               /* [n_cap][blk_stride] */
};

template <int FMT> void run_stage(const Emu *e, const K0Args &a, uint32_t *lds)
{
    if (e->resample) block_emu::run_block(WM_K0_THREADS, [&] { k0_resample_block_t<FMT, true, false, false, true>(a, lds); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_convert_block<FMT, true, false, false, true>(a, lds); });
}
template <int FMT> void run_gain(const Emu *e, const K0AgcArgs &g)
{
    if (e->R) block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, true>(g); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, false>(g); });
}
template <int FMT> void run_sums(const K0DcArgs &d) { block_emu::run_block(WM_K0_THREADS, [&] { k0_dc_sums_block<FMT>(d); }); }

#define BY_FORMAT(fmt, CALL) switch (fmt) { case WM_K0_CU8: CALL(WM_K0_CU8); break; case WM_K0_CS8: CALL(WM_K0_CS8); break; \
                                            case WM_K0_CS16: CALL(WM_K0_CS16); break; default: CALL(WM_K0_CF32); break; }
}

extern "C" {

/* taps == NULL: the conversion kernel (L = M = 1); tile: outputs per block (conversion: a multiple of 8); steps[n_ch] and table: what
 * wmbus_shift_design gave; R: cfg.input_dc (0: no blocker); agc: cfg.input_agc; max_blk: level blocks of the largest push (the row
 * length of the level tables, as cfg.max_push_bytes gives it to the library) */
void *wm_emu_ch_new(uint32_t fmt, uint32_t gain_q8, uint32_t L, uint32_t M, uint32_t T, const int16_t *taps, uint32_t tile, uint32_t n_cap,
                    uint32_t n_ch, const uint32_t *steps, const int16_t *table, uint32_t R, uint32_t agc, uint32_t max_blk)
{
    if (n_ch < 1u || n_ch > WM_K0_MAX_CH || n_cap < 1u) return nullptr;
    Emu *e = new Emu();
    e->fmt = fmt; e->gain = gain_q8; e->resample = taps != nullptr; e->R = R; e->agc = agc;
    e->L = taps ? L : 1u; e->M = taps ? M : 1u; e->T = taps ? T : 1u; e->tile = tile;
    e->n_cap = n_cap; e->n_ch = n_ch; e->S = n_cap * n_ch; e->blk_stride = max_blk;
    if (taps) e->taps.assign(taps, taps + (size_t)L * T);
    for (uint32_t c = 0; c < WM_K0_MAX_CH; c++) e->steps[c] = c < n_ch ? steps[c] : 0xDEADBEEFu;
    e->tab.resize(1024u);
    memcpy(e->tab.data(), table, 4096u);
    for (int i = 0; i < 2; i++) {
        e->hist[i].assign((size_t)e->S * e->T, 0u); e->rem_buf[i].assign((size_t)e->S * 4096u, 128u);
        e->st[i].assign(n_cap, K0DcState{0, 0, 0});
    }
    /* the tables and the sums hold what an earlier push left (the device buffers are never cleared) */
    e->sums.assign((size_t)n_cap * max_blk, K0S2{0x5A5A5A5A, 0x5A5A5A5A});
    e->dc_tab.assign((size_t)n_cap * max_blk, 0xDEADBEEFu);
    e->agc_tab.assign((size_t)n_cap * max_blk, (uint16_t)0xBEEFu);
    return e;
}
void wm_emu_ch_free(void *p) { delete (Emu *)p; }
unsigned wm_emu_ch_pick_tile(uint32_t L, uint32_t M, uint32_t T) { return k0_pick_tile(L, M, T); }
unsigned wm_emu_ch_convert_tile(uint32_t fmt) { return WM_K0_THREADS * WM_K0_CONV_UNROLL * (16u / k0_bps((int)fmt)); }
unsigned wm_emu_ch_max_channels(void) { return WM_K0_MAX_CH; }

/* One push of raw_bytes (multiple of 4096) of EVERY capture: raw = [n_cap][raw_stride].  windows = [n_cap * n_ch][window_stride], row v
 * receives the remainder of earlier pushes of pipeline stream v followed by this push's bytes.  Returns the bytes the pipeline would
 * take per stream (whole 4096-byte blocks); *clipped: the push's clip count, all channels of all captures. */
long wm_emu_ch_push(void *p, const uint8_t *raw, size_t raw_stride, size_t raw_bytes, uint8_t *windows, size_t window_stride, size_t window_cap,
                    uint32_t *clipped)
{
    Emu *e = (Emu *)p;
    const uint32_t n_in = (uint32_t)(raw_bytes / k0_bps((int)e->fmt));
    const uint64_t out_end = ((e->n_in + n_in) * (uint64_t)e->L + e->M - 1u) / e->M;
    const uint32_t n_out = (uint32_t)(out_end - e->n_out);
    const size_t total = (size_t)e->rem + 2u * (size_t)n_out, whole = total / 4096u * 4096u;
    const uint32_t n_blk = n_in >> WM_K0_DC_LOG2;
    if (total > window_cap || window_cap > window_stride || n_blk > e->blk_stride || raw_bytes > raw_stride) return -1;
    *clipped = 0u;
    K0DcArgs d{};
    d.raw = raw; d.raw_stride = raw_stride; d.sums = e->sums.data(); d.tab = e->dc_tab.data();
    d.st_in = e->st[e->cur].data(); d.st_out = e->st[e->cur ^ 1u].data();
    d.stride = e->blk_stride; d.n_blk = n_blk; d.R = e->R;
    if (e->R) {                                                  /* over captures, not over pipeline streams */
        gridDim = {(n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), e->n_cap, 1};
        for (uint32_t k = 0; k < e->n_cap; k++)
            for (uint32_t b = 0; b < gridDim.x; b++) {
                blockIdx = {b, k, 0};
#define CALL(F) run_sums<F>(d)
                BY_FORMAT(e->fmt, CALL)
#undef CALL
            }
        gridDim = {e->n_cap, 1, 1};
        for (uint32_t k = 0; k < e->n_cap; k++) {
            blockIdx = {k, 0, 0};
            int64_t slots[128];
            block_emu::run_block(128u, [&] { k0_dc_plan_block(d, slots); });
        }
    }
    if (e->agc) {
        K0AgcArgs g{};
        g.raw = raw; g.raw_stride = raw_stride; g.dc_tab = e->R ? e->dc_tab.data() : nullptr; g.tab = e->agc_tab.data();
        g.stride = e->blk_stride; g.n_blk = n_blk;
        gridDim = {(n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), e->n_cap, 1};
        for (uint32_t k = 0; k < e->n_cap; k++)
            for (uint32_t b = 0; b < gridDim.x; b++) {
                blockIdx = {b, k, 0};
#define CALL(F) run_gain<F>(e, g)
                BY_FORMAT(e->fmt, CALL)
#undef CALL
            }
    }
    e->last_blk = n_blk;

    K0Args a{};
    a.raw = raw; a.raw_stride = raw_stride; a.out = windows; a.out_stride = window_stride; a.taps = e->taps.data();
    /* rows of T - 1 samples, as the library lays them out (the conversion kernel has no history: T = 1) */
    a.hist_in = e->hist[e->cur].data(); a.hist_out = e->hist[e->cur ^ 1u].data();
    a.rem_in = e->rem_buf[e->cur].data(); a.rem_out = e->rem_buf[e->cur ^ 1u].data();
    a.n_first = e->n_out; a.in_first = e->n_in; a.n_in = n_in; a.n_out = n_out;
    a.rem_prev = e->rem; a.keep_from = (uint32_t)whole;
    a.L = e->L; a.M = e->M; a.T = e->T; a.tile = e->tile;
    a.gain_q8 = e->gain; a.clipped = clipped;
    a.step = 0xDEADBEEFu;                                        /* the channels form must not look at the single shift's step */
    a.shift_tab = e->tab.data();
    a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.agc_tab = e->agc ? e->agc_tab.data() : nullptr; a.dc_stride = e->blk_stride;
    a.n_ch = e->n_ch;
    for (uint32_t c = 0; c < WM_K0_MAX_CH; c++) a.steps[c] = e->steps[c];
    std::vector<uint32_t> lds((e->resample ? k0_lds_bytes(e->L, e->M, e->T, e->tile) : 4u) / 4u + 1u);
    gridDim = {(n_out + e->tile - 1u) / e->tile, e->S, 1};
    for (uint32_t v = 0; v < e->S; v++)
        for (uint32_t b = 0; b < gridDim.x; b++) {
            blockIdx = {b, v, 0};
            std::fill(lds.begin(), lds.end(), 0xDEADBEEFu);      /* what a block finds in LDS is not defined */
#define CALL(F) run_stage<F>(e, a, lds.data())
            BY_FORMAT(e->fmt, CALL)
#undef CALL
        }
    e->n_in += n_in; e->n_out = out_end; e->rem = (uint32_t)(total - whole); e->cur ^= 1u;
    return (long)whole;
}

/* {dc_I, dc_Q} / g of the last push's level blocks of one CAPTURE, as wmbus_read_input_dc / wmbus_read_input_gain give them */
long wm_emu_ch_read_dc(void *p, uint32_t capture, int16_t *iq, size_t cap_pairs)
{
    Emu *e = (Emu *)p;
    if (capture >= e->n_cap) return -1;
    const size_t n = std::min<size_t>(cap_pairs, e->last_blk);
    memcpy(iq, e->dc_tab.data() + (size_t)capture * e->blk_stride, 4u * n);
    return (long)n;
}
long wm_emu_ch_read_gain(void *p, uint32_t capture, uint16_t *g, size_t cap)
{
    Emu *e = (Emu *)p;
    if (capture >= e->n_cap) return -1;
    const size_t n = std::min<size_t>(cap, e->last_blk);
    memcpy(g, e->agc_tab.data() + (size_t)capture * e->blk_stride, 2u * n);
    return (long)n;
}

}
