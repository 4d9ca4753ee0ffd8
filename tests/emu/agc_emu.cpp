/* agc_emu.cpp -- TEST INFRASTRUCTURE: the per-block AGC of K0 (device source wm_k0_resample.h: k0_agc_gain_block<FMT, DC> and the AG
 * instantiations k0_resample_block_t<FMT, SH, DC, true> / k0_convert_block<FMT, SH, DC, true>, what k0_agc_gain<>, k0_resample_agc<> and
 * k0_convert_agc<> run) on the coroutine block emulator, driven push by push the way wm_api.hip drives the kernels: with a blocker its
 * sums and its plan, then the gain, then the K0 kernel, with the same launch arguments, the same double-buffered carried state (history,
 * remainder, the blocker's), the clip counter zeroed per push.  The twin of dc_emu.cpp. */
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
    uint32_t fmt, gain, L, M, T, tile, step, R, cur = 0, rem = 0, last_blk = 0;
    bool resample, shift;
    uint64_t n_in = 0, n_out = 0;
    std::vector<int16_t> taps;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    std::vector<uint32_t> hist[2];
    std::vector<uint8_t> rem_buf[2];
    K0DcState st[2] = {{0, 0, 0}, {0, 0, 0}};
    std::vector<K0S2> sums;
    std::vector<uint32_t> dc_tab;
    std::vector<uint16_t> agc_tab;
};

template <int FMT, bool SH, bool DC> void run_k0(const Emu *e, const K0Args &a, uint32_t *lds)
{
    if (e->resample) block_emu::run_block(WM_K0_THREADS, [&] { k0_resample_block_t<FMT, SH, DC, true>(a, lds); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_convert_block<FMT, SH, DC, true>(a, lds); });
}
template <int FMT, bool SH> void run_sh(const Emu *e, const K0Args &a, uint32_t *lds)
{
    if (e->R) run_k0<FMT, SH, true>(e, a, lds); else run_k0<FMT, SH, false>(e, a, lds);
}
template <int FMT> void run_fmt(const Emu *e, const K0Args &a, uint32_t *lds)
{
    if (e->shift) run_sh<FMT, true>(e, a, lds); else run_sh<FMT, false>(e, a, lds);
}
template <int FMT> void run_gain(const Emu *e, const K0AgcArgs &g)
{
    if (e->R) block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, true>(g); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, false>(g); });
}
template <int FMT> void run_sums(const K0DcArgs &d) { block_emu::run_block(WM_K0_THREADS, [&] { k0_dc_sums_block<FMT>(d); }); }
}

extern "C" {

/* taps == NULL: the conversion kernel (L = M = 1); tile: outputs per block (conversion: a multiple of 8); table == NULL: no shift, else
 * step and table are what wmbus_shift_design gave (1024 x {c, s}); R: cfg.input_dc (0: no blocker); the gain is the AGC's */
void *wm_emu_agc_new(uint32_t fmt, uint32_t gain_q8, uint32_t L, uint32_t M, uint32_t T, const int16_t *taps, uint32_t tile, uint32_t step,
                    const int16_t *table, uint32_t R)
{
    Emu *e = new Emu();
    e->fmt = fmt; e->gain = gain_q8; e->resample = taps != nullptr; e->shift = table != nullptr; e->R = R;
    e->L = taps ? L : 1u; e->M = taps ? M : 1u; e->T = taps ? T : 1u; e->tile = tile;
    if (taps) e->taps.assign(taps, taps + (size_t)L * T);
    e->step = step;
    if (table) { e->tab.resize(1024u); memcpy(e->tab.data(), table, 4096u); }
    for (int i = 0; i < 2; i++) { e->hist[i].assign(e->T, 0u); e->rem_buf[i].assign(4096u, 128u); }
    return e;
}
void wm_emu_agc_free(void *p) { delete (Emu *)p; }
unsigned wm_emu_agc_pick_tile(uint32_t L, uint32_t M, uint32_t T) { return k0_pick_tile(L, M, T); }
unsigned wm_emu_agc_convert_tile(uint32_t fmt) { return WM_K0_THREADS * WM_K0_CONV_UNROLL * (16u / k0_bps((int)fmt)); }

/* One push of raw_bytes (multiple of 4096) of one capture.  window: receives the remainder of earlier pushes followed by this
 * push's bytes.  Returns the bytes the pipeline would take (whole 4096-byte blocks); *clipped: the push's clip count. */
long wm_emu_agc_push(void *p, const uint8_t *raw, size_t raw_bytes, uint8_t *window, size_t window_cap, uint32_t *clipped)
{
    Emu *e = (Emu *)p;
    const uint32_t n_in = (uint32_t)(raw_bytes / k0_bps((int)e->fmt));
    const uint64_t out_end = ((e->n_in + n_in) * (uint64_t)e->L + e->M - 1u) / e->M;
    const uint32_t n_out = (uint32_t)(out_end - e->n_out);
    const size_t total = (size_t)e->rem + 2u * (size_t)n_out, whole = total / 4096u * 4096u;
    if (total > window_cap) return -1;
    *clipped = 0u;
    /* the tables and the sums hold what an earlier push left (the device buffers are never cleared) and have no room to spare */
    const uint32_t n_blk = n_in >> WM_K0_DC_LOG2;
    e->sums.resize(std::max<size_t>(e->sums.size(), n_blk), K0S2{0x5A5A5A5A, 0x5A5A5A5A});
    e->dc_tab.resize(std::max<size_t>(e->dc_tab.size(), n_blk), 0xDEADBEEFu);
    e->agc_tab.resize(std::max<size_t>(e->agc_tab.size(), n_blk), (uint16_t)0xBEEFu);
    K0DcArgs d{};
    d.raw = raw; d.raw_stride = 0; d.sums = e->sums.data(); d.tab = e->dc_tab.data();
    d.st_in = &e->st[e->cur]; d.st_out = &e->st[e->cur ^ 1u];
    d.stride = (uint32_t)e->sums.size(); d.n_blk = n_blk; d.R = e->R;
    if (e->R) {
        gridDim = {(n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), 1, 1};
        for (uint32_t b = 0; b < gridDim.x; b++) {
            blockIdx = {b, 0, 0};
            switch (e->fmt) {
            case WM_K0_CU8: run_sums<WM_K0_CU8>(d); break;
            case WM_K0_CS8: run_sums<WM_K0_CS8>(d); break;
            case WM_K0_CS16: run_sums<WM_K0_CS16>(d); break;
            default: run_sums<WM_K0_CF32>(d); break;
            }
        }
        gridDim = {1, 1, 1}; blockIdx = {0, 0, 0};
        int64_t slots[128];
        block_emu::run_block(128u, [&] { k0_dc_plan_block(d, slots); });
    }
    K0AgcArgs g{};
    g.raw = raw; g.raw_stride = 0; g.dc_tab = e->R ? e->dc_tab.data() : nullptr; g.tab = e->agc_tab.data();
    g.stride = d.stride; g.n_blk = n_blk;
    gridDim = {(n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) {
        blockIdx = {b, 0, 0};
        switch (e->fmt) {
        case WM_K0_CU8: run_gain<WM_K0_CU8>(e, g); break;
        case WM_K0_CS8: run_gain<WM_K0_CS8>(e, g); break;
        case WM_K0_CS16: run_gain<WM_K0_CS16>(e, g); break;
        default: run_gain<WM_K0_CF32>(e, g); break;
        }
    }
    e->last_blk = n_blk;

    K0Args a{};
    a.raw = raw; a.raw_stride = 0; a.out = window; a.out_stride = 0; a.taps = e->taps.data();
    a.hist_in = e->hist[e->cur].data(); a.hist_out = e->hist[e->cur ^ 1u].data();
    a.rem_in = e->rem_buf[e->cur].data(); a.rem_out = e->rem_buf[e->cur ^ 1u].data();
    a.n_first = e->n_out; a.in_first = e->n_in; a.n_in = n_in; a.n_out = n_out;
    a.rem_prev = e->rem; a.keep_from = (uint32_t)whole;
    a.L = e->L; a.M = e->M; a.T = e->T; a.tile = e->tile;
    a.gain_q8 = e->gain; a.clipped = clipped;
    a.step = e->step; a.shift_tab = e->shift ? e->tab.data() : nullptr;
    a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.dc_stride = d.stride; a.agc_tab = e->agc_tab.data();
    std::vector<uint32_t> lds((e->resample ? k0_lds_bytes(e->L, e->M, e->T, e->tile) : 4u) / 4u + 1u);
    gridDim = {(n_out + e->tile - 1u) / e->tile, 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) {
        blockIdx = {b, 0, 0};
        std::fill(lds.begin(), lds.end(), 0xDEADBEEFu);          /* what a block finds in LDS is not defined */
        switch (e->fmt) {
        case WM_K0_CU8: run_fmt<WM_K0_CU8>(e, a, lds.data()); break;
        case WM_K0_CS8: run_fmt<WM_K0_CS8>(e, a, lds.data()); break;
        case WM_K0_CS16: run_fmt<WM_K0_CS16>(e, a, lds.data()); break;
        default: run_fmt<WM_K0_CF32>(e, a, lds.data()); break;
        }
    }
    e->n_in += n_in; e->n_out = out_end; e->rem = (uint32_t)(total - whole); e->cur ^= 1u;
    return (long)whole;
}

/* g of the last push's level blocks, as wmbus_read_input_gain gives them; returns the values written */
long wm_emu_agc_read(void *p, uint16_t *g, size_t cap)
{
    Emu *e = (Emu *)p;
    const size_t n = std::min<size_t>(cap, e->last_blk);
    memcpy(g, e->agc_tab.data(), 2u * n);
    return (long)n;
}

}
