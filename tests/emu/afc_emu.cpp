/* afc_emu.cpp -- TEST INFRASTRUCTURE: automatic frequency correction of K0 on the coroutine block emulator, in its two parts.
 *   wm_emu_afc_plan   the device source of k0_afc_plan (wm_k0_afc.h: k0_afc_plan_block) for one capture: a max-hold, a block count and a
 *                     state in, {step, base} of the push and the next state out -- one block of 512 threads, the launch wm_api.hip makes.
 *   wm_emu_afc_*      the AFC form of the two stage kernels (wm_k0_resample.h: k0_resample_block_t<FMT, true, false, false, false, true> and
 *                     k0_convert_block<FMT, true, false, false, false, true>, what k0_resample_afc<> and k0_convert_afc<> run, behind
 *                     k0_dc_sums / k0_dc_plan / k0_agc_gain where the blocker or the AGC is on), driven push by push the way wm_api.hip drives
 *                     them, with the {step, base} of every capture and push SCRIPTED by the caller: the table k0_afc_plan would have left.
 * The twin of channels_emu.cpp. */
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

#include "wm_k0_afc.h"

namespace {
struct Emu {
    uint32_t fmt, gain, L, M, T, tile, n_cap, R, agc, blk_stride, cur = 0, rem = 0;
    bool resample;
    uint64_t n_in = 0, n_out = 0;
    std::vector<int16_t> taps;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    std::vector<uint32_t> hist[2];                               /* [n_cap][T - 1] */
    std::vector<uint8_t> rem_buf[2];                             /* [n_cap][4096] */
    std::vector<K0DcState> st[2];                                /* [n_cap] */
    std::vector<K0S2> sums;                                      /* [n_cap][blk_stride] */
    std::vector<uint32_t> dc_tab;                                /* [n_cap][blk_stride] */
    std::vector<uint16_t> agc_tab;                               /* [n_cap][blk_stride] */
};

template <int FMT> void run_stage(const Emu *e, const K0Args &a, uint32_t *lds)
{
    if (e->resample) block_emu::run_block(WM_K0_THREADS, [&] { k0_resample_block_t<FMT, true, false, false, false, true>(a, lds); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_convert_block<FMT, true, false, false, false, true>(a, lds); });
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

unsigned wm_emu_afc_state_bytes(void) { return (unsigned)sizeof(K0AfcState); }

/* k0_afc_plan for one capture.  state: {held_hz, locked, changes, ratio_q8, base} in and out; push_out: {step, base} of this push.  The
 * capture sits at index `at` of `n_cap` (the others hold garbage): a stride mix-up shows. */
void wm_emu_afc_plan(uint32_t in_hz, int32_t nominal_hz, uint32_t range_hz, const uint32_t *peak, uint64_t blocks, uint32_t n_in, uint32_t *state,
                     uint32_t *push_out, uint32_t at, uint32_t n_cap)
{
    std::vector<uint32_t> pk((size_t)n_cap * WM_K0_SPEC_BINS, 0xDEADBEEFu);
    std::vector<uint64_t> blk(n_cap, 0x5A5A5A5A5A5A5A5Aull);
    std::vector<K0AfcState> in(n_cap, K0AfcState{0x5A5A5A5A, 0x5Au, 0x5Au, 0x5Au, 0x5Au, {0u, 0u, 0u}}), out(n_cap, in[0]);
    std::vector<K0AfcPush> push(n_cap, K0AfcPush{0xDEADBEEFu, 0xDEADBEEFu});
    memcpy(pk.data() + (size_t)at * WM_K0_SPEC_BINS, peak, 4u * WM_K0_SPEC_BINS);
    blk[at] = blocks;
    in[at] = K0AfcState{(int32_t)state[0], state[1], state[2], state[3], state[4], {0u, 0u, 0u}};
    const K0AfcArgs a{pk.data(), blk.data(), in.data(), out.data(), push.data(), in_hz, nominal_hz, range_hz, n_in};
    K0AfcLds *lds = new K0AfcLds;
    memset(lds, 0xA5, sizeof *lds);                              /* what a block finds in LDS is not defined */
    gridDim = {n_cap, 1, 1}; blockIdx = {at, 0, 0};
    block_emu::run_block(WM_K0_AFC_THREADS, [&] { k0_afc_plan_block(a, *lds); });
    delete lds;
    state[0] = (uint32_t)out[at].held_hz; state[1] = out[at].locked; state[2] = out[at].changes; state[3] = out[at].ratio_q8; state[4] = out[at].base;
    push_out[0] = push[at].step; push_out[1] = push[at].base;
}

/* taps == NULL: the conversion kernel (L = M = 1); tile: outputs per block (conversion: a multiple of 8); table: what wmbus_shift_design
 * gave; R: cfg.input_dc (0: no blocker); agc: cfg.input_agc; max_blk: level blocks of the largest push */
void *wm_emu_afc_new(uint32_t fmt, uint32_t gain_q8, uint32_t L, uint32_t M, uint32_t T, const int16_t *taps, uint32_t tile, uint32_t n_cap,
                     const int16_t *table, uint32_t R, uint32_t agc, uint32_t max_blk)
{
    if (n_cap < 1u) return nullptr;
    Emu *e = new Emu();
    e->fmt = fmt; e->gain = gain_q8; e->resample = taps != nullptr; e->R = R; e->agc = agc;
    e->L = taps ? L : 1u; e->M = taps ? M : 1u; e->T = taps ? T : 1u; e->tile = tile;
    e->n_cap = n_cap; e->blk_stride = max_blk;
    if (taps) e->taps.assign(taps, taps + (size_t)L * T);
    e->tab.resize(1024u);
    memcpy(e->tab.data(), table, 4096u);
    for (int i = 0; i < 2; i++) {
        e->hist[i].assign((size_t)n_cap * e->T, 0u); e->rem_buf[i].assign((size_t)n_cap * 4096u, 128u);
        e->st[i].assign(n_cap, K0DcState{0, 0, 0});
    }
    e->sums.assign((size_t)n_cap * max_blk, K0S2{0x5A5A5A5A, 0x5A5A5A5A});
    e->dc_tab.assign((size_t)n_cap * max_blk, 0xDEADBEEFu);
    e->agc_tab.assign((size_t)n_cap * max_blk, (uint16_t)0xBEEFu);
    return e;
}
void wm_emu_afc_free(void *p) { delete (Emu *)p; }
unsigned wm_emu_afc_pick_tile(uint32_t L, uint32_t M, uint32_t T) { return k0_pick_tile(L, M, T); }
unsigned wm_emu_afc_convert_tile(uint32_t fmt) { return WM_K0_THREADS * WM_K0_CONV_UNROLL * (16u / k0_bps((int)fmt)); }

/* One push of raw_bytes (multiple of 4096) of EVERY capture: raw = [n_cap][raw_stride]; plan = [n_cap] {step, base}, what k0_afc_plan
 * left for this push.  windows = [n_cap][window_stride], row k receives the remainder of earlier pushes of capture k followed by this
 * push's bytes.  Returns the bytes the pipeline would take per capture (whole 4096-byte blocks); *clipped: the push's clip count. */
long wm_emu_afc_push(void *p, const uint8_t *raw, size_t raw_stride, size_t raw_bytes, const uint32_t *plan, uint8_t *windows, size_t window_stride,
                     size_t window_cap, uint32_t *clipped)
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
    if (e->R) {
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
    std::vector<K0AfcPush> push(e->n_cap);
    for (uint32_t k = 0; k < e->n_cap; k++) push[k] = K0AfcPush{plan[2u * k], plan[2u * k + 1u]};

    K0Args a{};
    a.raw = raw; a.raw_stride = raw_stride; a.out = windows; a.out_stride = window_stride; a.taps = e->taps.data();
    a.hist_in = e->hist[e->cur].data(); a.hist_out = e->hist[e->cur ^ 1u].data();
    a.rem_in = e->rem_buf[e->cur].data(); a.rem_out = e->rem_buf[e->cur ^ 1u].data();
    a.n_first = e->n_out; a.in_first = e->n_in; a.n_in = n_in; a.n_out = n_out;
    a.rem_prev = e->rem; a.keep_from = (uint32_t)whole;
    a.L = e->L; a.M = e->M; a.T = e->T; a.tile = e->tile;
    a.gain_q8 = e->gain; a.clipped = clipped;
    a.step = 0xDEADBEEFu;                                        /* the AFC form must not look at the single shift's step, nor at the channels' */
    a.n_ch = 0xDEADBEEFu;
    for (uint32_t c = 0; c < WM_K0_MAX_CH; c++) a.steps[c] = 0xDEADBEEFu;
    a.shift_tab = e->tab.data();
    a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.agc_tab = e->agc ? e->agc_tab.data() : nullptr; a.dc_stride = e->blk_stride;
    a.afc = push.data();
    std::vector<uint32_t> lds((e->resample ? k0_lds_bytes(e->L, e->M, e->T, e->tile) : 4u) / 4u + 1u);
    gridDim = {(n_out + e->tile - 1u) / e->tile, e->n_cap, 1};
    for (uint32_t v = 0; v < e->n_cap; v++)
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

}
