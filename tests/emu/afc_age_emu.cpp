/* afc_age_emu.cpp -- TEST INFRASTRUCTURE: the survey that forgets (cfg.input_spectrum_age) on the coroutine block emulator.
 *   wm_emu_age_*          the AGE form of the survey kernel (device source wm_k0_spectrum.h: k0_spectrum_block<FMT, DC, true>, what
 *                         k0_spectrum<FMT, DC, true> runs) driven push by push the way wm_api.hip drives it: with a blocker its sums and its
 *                         plan first, then k0_spec_age_plan -- the library's own decision of what the push clears and leaves out, the very
 *                         function wm_api.hip calls -- the fills it asks for, and the kernel over the push's level blocks into the two slots,
 *                         laid out as the library lays them out ({sum | blocks | peak} per slot, slot 1 a stride behind slot 0).
 *   wm_emu_age_host_plan  k0_spec_age_plan on its own.
 *   wm_emu_age_afc_plan   the device source of k0_afc_plan (wm_k0_afc.h: k0_afc_plan_block) on the two slots of a capture.
 * And the lock per channel (cfg.input_channel_afc_hz):
 *   wm_emu_chafc_plan     k0_afc_plan_block on the grid (captures, channels) wm_api.hip launches for a channel list: the max-hold of
 *                         every capture in, the state and {step, base} of every pipeline stream v = capture x channels + channel out.
 *   wm_emu_chafc_*        the CH && AF form of the two stage kernels (wm_k0_resample.h: k0_resample_block_t<FMT, true, false, false, true,
 *                         true> and k0_convert_block<FMT, true, false, false, true, true>, what k0_resample_ch_afc<> and k0_convert_ch_afc<>
 *                         run), driven push by push with the {step, base} of every v SCRIPTED by the caller.
 * The twin of spectrum_emu.cpp, afc_emu.cpp and channels_emu.cpp. */
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
constexpr uint64_t STRIDE = WM_K0_SPEC_BINS + 1u + WM_K0_SPEC_BINS / 2u;      /* one capture: wm_api.hip's slot */

struct Emu {
    uint32_t fmt, R, run, age, cur = 0;
    uint64_t K = 0;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    K0DcState st[2] = {{0, 0, 0}, {0, 0, 0}};
    std::vector<K0S2> sums;
    std::vector<uint32_t> dc_tab;
    uint64_t slots[2 * STRIDE];
    uint64_t *sum(unsigned s) { return slots + s * STRIDE; }
    uint64_t *blocks(unsigned s) { return slots + s * STRIDE + WM_K0_SPEC_BINS; }
    uint32_t *peak(unsigned s) { return (uint32_t *)(slots + WM_K0_SPEC_BINS + 1u) + 2u * s * STRIDE; }
};

template <int FMT> void run_sums(const K0DcArgs &d) { block_emu::run_block(WM_K0_THREADS, [&] { k0_dc_sums_block<FMT>(d); }); }
template <int FMT> void run_spec(const Emu *e, const K0SpecArgs &a, int32_t *lds)
{
    if (e->R) block_emu::run_block(64u * WM_K0_SPEC_WAVES, [&] { k0_spectrum_block<FMT, true, true>(a, lds); });
    else block_emu::run_block(64u * WM_K0_SPEC_WAVES, [&] { k0_spectrum_block<FMT, false, true>(a, lds); });
}

struct ChEmu {
    uint32_t fmt, gain, L, M, T, tile, n_cap, n_ch, R, agc, blk_stride, cur = 0, rem = 0;
    bool resample;
    uint64_t n_in = 0, n_out = 0;
    std::vector<int16_t> taps;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    std::vector<uint32_t> hist[2];                               /* [n_cap x n_ch][T - 1] */
    std::vector<uint8_t> rem_buf[2];                             /* [n_cap x n_ch][4096] */
    std::vector<K0DcState> st[2];                                /* [n_cap] */
    std::vector<K0S2> sums;                                      /* [n_cap][blk_stride] */
    std::vector<uint32_t> dc_tab;                                /* [n_cap][blk_stride] */
    std::vector<uint16_t> agc_tab;                               /* [n_cap][blk_stride] */
};

template <int FMT> void run_ch_stage(const ChEmu *e, const K0Args &a, uint32_t *lds)
{
    if (e->resample) block_emu::run_block(WM_K0_THREADS, [&] { k0_resample_block_t<FMT, true, false, false, true, true>(a, lds); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_convert_block<FMT, true, false, false, true, true>(a, lds); });
}
template <int FMT> void run_ch_gain(const ChEmu *e, const K0AgcArgs &g)
{
    if (e->R) block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, true>(g); });
    else block_emu::run_block(WM_K0_THREADS, [&] { k0_agc_gain_block<FMT, false>(g); });
}

#define BY_FORMAT(fmt, CALL) switch (fmt) { case WM_K0_CU8: CALL(WM_K0_CU8); break; case WM_K0_CS8: CALL(WM_K0_CS8); break; \
                                            case WM_K0_CS16: CALL(WM_K0_CS16); break; default: CALL(WM_K0_CF32); break; }
}

extern "C" {

void wm_emu_age_host_plan(uint64_t k_first, uint32_t n_blk, uint32_t age, uint64_t *e_keep, uint32_t *clear)
{
    const K0SpecAgePlan p = k0_spec_age_plan(k_first, n_blk, age);
    *e_keep = p.e_keep; *clear = p.clear;
}

/* table: what wmbus_shift_design gave (1024 x {c, s}); R: cfg.input_dc (0: no blocker); run: level blocks per wave; age: A;
 * k_start: the stream's index of the first level block this emulator will see (a context that has run for long: the 64 bits of K) --
 * the slots start clear */
void *wm_emu_age_new(uint32_t fmt, const int16_t *table, uint32_t R, uint32_t run, uint32_t age, uint64_t k_start)
{
    Emu *e = new Emu();
    e->fmt = fmt; e->R = R; e->run = run; e->age = age; e->K = k_start;
    e->tab.resize(1024u); memcpy(e->tab.data(), table, 4096u);
    memset(e->slots, 0, sizeof e->slots);
    return e;
}
void wm_emu_age_free(void *p) { delete (Emu *)p; }

/* One push of raw_bytes (multiple of 4096) of one capture.  Returns the level blocks of the push. */
long wm_emu_age_push(void *p, const uint8_t *raw, size_t raw_bytes)
{
    Emu *e = (Emu *)p;
    const uint32_t n_blk = (uint32_t)(raw_bytes / k0_bps((int)e->fmt)) >> WM_K0_DC_LOG2;
    if (!n_blk) return 0;
    if (e->R) {
        e->sums.resize(std::max<size_t>(e->sums.size(), n_blk), K0S2{0x5A5A5A5A, 0x5A5A5A5A});
        e->dc_tab.resize(std::max<size_t>(e->dc_tab.size(), n_blk), 0xDEADBEEFu);
        K0DcArgs d{};
        d.raw = raw; d.raw_stride = 0; d.sums = e->sums.data(); d.tab = e->dc_tab.data();
        d.st_in = &e->st[e->cur]; d.st_out = &e->st[e->cur ^ 1u];
        d.stride = (uint32_t)e->sums.size(); d.n_blk = n_blk; d.R = e->R;
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
        e->cur ^= 1u;
    }
    const K0SpecAgePlan plan = k0_spec_age_plan(e->K, n_blk, e->age);
    for (unsigned s = 0; s < 2u; s++)
        if (plan.clear >> s & 1u) memset(e->slots + s * STRIDE, 0, STRIDE * sizeof(uint64_t));
    K0SpecArgs a{};
    a.raw = raw; a.raw_stride = 0; a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.dc_stride = (uint32_t)e->dc_tab.size();
    a.shift_tab = e->tab.data(); a.sum = e->sum(0); a.peak = e->peak(0); a.blocks = e->blocks(0);
    a.n_blk = n_blk; a.run = e->run;
    a.age = e->age; a.k_first = e->K; a.e_keep = plan.e_keep; a.slot_stride = STRIDE;
    e->K += n_blk;
    std::vector<int32_t> lds(WM_K0_SPEC_WAVES * 2u * WM_K0_SPEC_PLANE);
    const uint32_t runs = (n_blk + e->run - 1u) / e->run;
    gridDim = {(runs + WM_K0_SPEC_WAVES - 1u) / WM_K0_SPEC_WAVES, 1, 1};
    for (uint32_t b = 0; b < gridDim.x; b++) {
        blockIdx = {b, 0, 0};
        std::fill(lds.begin(), lds.end(), (int32_t)0xDEADBEEF);  /* what a block finds in LDS is not defined */
        switch (e->fmt) {
        case WM_K0_CU8: run_spec<WM_K0_CU8>(e, a, lds.data()); break;
        case WM_K0_CS8: run_spec<WM_K0_CS8>(e, a, lds.data()); break;
        case WM_K0_CS16: run_spec<WM_K0_CS16>(e, a, lds.data()); break;
        default: run_spec<WM_K0_CF32>(e, a, lds.data()); break;
        }
    }
    return (long)n_blk;
}

/* as wmbus_read_spectrum on an ageing context: the view, the two slots together; reset != 0 empties both behind the read */
long wm_emu_age_read(void *p, uint64_t *sum, uint32_t *peak, uint64_t *blocks, int reset)
{
    Emu *e = (Emu *)p;
    for (unsigned b = 0; b < WM_K0_SPEC_BINS; b++) {
        if (sum) sum[b] = e->sum(0)[b] + e->sum(1)[b];
        if (peak) peak[b] = std::max(e->peak(0)[b], e->peak(1)[b]);
    }
    if (blocks) *blocks = *e->blocks(0) + *e->blocks(1);
    if (reset) memset(e->slots, 0, sizeof e->slots);
    return (long)WM_K0_SPEC_BINS;
}

/* the level blocks each slot holds (the view's parts) */
void wm_emu_age_slot_blocks(void *p, uint64_t *out) { Emu *e = (Emu *)p; out[0] = *e->blocks(0); out[1] = *e->blocks(1); }

/* k0_afc_plan on the emulator's two slots, the capture at index `at` of `n_cap` (the others hold garbage, in both slots).  state:
 * {held_hz, locked, changes, ratio_q8, base} in and out; push_out: {step, base} of this push. */
void wm_emu_age_afc_plan(void *p, uint32_t in_hz, int32_t nominal_hz, uint32_t range_hz, uint32_t n_in, uint32_t *state, uint32_t *push_out, uint32_t at,
                         uint32_t n_cap)
{
    Emu *e = (Emu *)p;
    std::vector<uint32_t> pk[2];
    std::vector<uint64_t> blk[2];
    for (unsigned s = 0; s < 2u; s++) {
        pk[s].assign((size_t)n_cap * WM_K0_SPEC_BINS, 0xDEADBEEFu);
        blk[s].assign(n_cap, 0x5A5A5A5A5A5A5A5Aull);
        memcpy(pk[s].data() + (size_t)at * WM_K0_SPEC_BINS, e->peak(s), 4u * WM_K0_SPEC_BINS);
        blk[s][at] = *e->blocks(s);
    }
    std::vector<K0AfcState> in(n_cap, K0AfcState{0x5A5A5A5A, 0x5Au, 0x5Au, 0x5Au, 0x5Au, {0u, 0u, 0u}}), out(n_cap, in[0]);
    std::vector<K0AfcPush> push(n_cap, K0AfcPush{0xDEADBEEFu, 0xDEADBEEFu});
    in[at] = K0AfcState{(int32_t)state[0], state[1], state[2], state[3], state[4], {0u, 0u, 0u}};
    K0AfcArgs a{};
    a.peak = pk[0].data(); a.blocks = blk[0].data(); a.st_in = in.data(); a.st_out = out.data(); a.push = push.data();
    a.in_hz = in_hz; a.nominal_hz = nominal_hz; a.range_hz = range_hz; a.n_in = n_in;
    a.peak1 = pk[1].data(); a.blocks1 = blk[1].data();
    K0AfcLds *lds = new K0AfcLds;
    memset(lds, 0xA5, sizeof *lds);                              /* what a block finds in LDS is not defined */
    gridDim = {n_cap, 1, 1}; blockIdx = {at, 0, 0};
    block_emu::run_block(WM_K0_AFC_THREADS, [&] { k0_afc_plan_block(a, *lds); });
    delete lds;
    state[0] = (uint32_t)out[at].held_hz; state[1] = out[at].locked; state[2] = out[at].changes; state[3] = out[at].ratio_q8; state[4] = out[at].base;
    push_out[0] = push[at].step; push_out[1] = push[at].base;
}

/* k0_afc_plan for a channel list: peaks = [n_cap][512], blocks = [n_cap]; nominal / range = [n_ch]; states = [n_cap x n_ch][5] {held_hz,
 * locked, changes, ratio_q8, base} in and out; push_out = [n_cap x n_ch][2] {step, base}.  The single-capture arguments hold garbage. */
void wm_emu_chafc_plan(uint32_t in_hz, uint32_t n_cap, uint32_t n_ch, const int32_t *nominal, const uint32_t *range, const uint32_t *peaks, const uint64_t *blocks,
                       uint32_t n_in, uint32_t *states, uint32_t *push_out)
{
    const uint32_t nv = n_cap * n_ch;
    std::vector<K0AfcState> in(nv), out(nv, K0AfcState{0x5A5A5A5A, 0x5Au, 0x5Au, 0x5Au, 0x5Au, {0u, 0u, 0u}});
    std::vector<K0AfcPush> push(nv, K0AfcPush{0xDEADBEEFu, 0xDEADBEEFu});
    for (uint32_t v = 0; v < nv; v++) in[v] = K0AfcState{(int32_t)states[5u * v], states[5u * v + 1u], states[5u * v + 2u], states[5u * v + 3u], states[5u * v + 4u], {0u, 0u, 0u}};
    K0AfcArgs a{};
    a.peak = peaks; a.blocks = blocks; a.st_in = in.data(); a.st_out = out.data(); a.push = push.data();
    a.in_hz = in_hz; a.nominal_hz = 0x5A5A5A5A; a.range_hz = 0x5A5A5A5Au; a.n_in = n_in;
    a.n_ch = n_ch;
    for (uint32_t c = 0; c < n_ch; c++) { a.ch_nominal_hz[c] = nominal[c]; a.ch_range_hz[c] = range[c]; }
    K0AfcLds *lds = new K0AfcLds;
    gridDim = {n_cap, n_ch, 1};
    for (uint32_t k = 0; k < n_cap; k++)
        for (uint32_t c = 0; c < n_ch; c++) {
            memset(lds, 0xA5, sizeof *lds);                      /* what a block finds in LDS is not defined */
            blockIdx = {k, c, 0};
            block_emu::run_block(WM_K0_AFC_THREADS, [&] { k0_afc_plan_block(a, *lds); });
        }
    delete lds;
    blockIdx = {0, 0, 0};
    for (uint32_t v = 0; v < nv; v++) {
        states[5u * v] = (uint32_t)out[v].held_hz; states[5u * v + 1u] = out[v].locked; states[5u * v + 2u] = out[v].changes;
        states[5u * v + 3u] = out[v].ratio_q8; states[5u * v + 4u] = out[v].base;
        push_out[2u * v] = push[v].step; push_out[2u * v + 1u] = push[v].base;
    }
}

/* taps == NULL: the conversion kernel (L = M = 1); tile: outputs per block; table: what wmbus_shift_design gave; R: cfg.input_dc; agc:
 * cfg.input_agc; max_blk: level blocks of the largest push */
void *wm_emu_chafc_new(uint32_t fmt, uint32_t gain_q8, uint32_t L, uint32_t M, uint32_t T, const int16_t *taps, uint32_t tile, uint32_t n_cap, uint32_t n_ch,
                       const int16_t *table, uint32_t R, uint32_t agc, uint32_t max_blk)
{
    if (n_cap < 1u || n_ch < 1u || n_ch > WM_K0_MAX_CH) return nullptr;
    ChEmu *e = new ChEmu();
    e->fmt = fmt; e->gain = gain_q8; e->resample = taps != nullptr; e->R = R; e->agc = agc;
    e->L = taps ? L : 1u; e->M = taps ? M : 1u; e->T = taps ? T : 1u; e->tile = tile;
    e->n_cap = n_cap; e->n_ch = n_ch; e->blk_stride = max_blk;
    if (taps) e->taps.assign(taps, taps + (size_t)L * T);
    e->tab.resize(1024u);
    memcpy(e->tab.data(), table, 4096u);
    for (int i = 0; i < 2; i++) {
        e->hist[i].assign((size_t)n_cap * n_ch * e->T, 0u); e->rem_buf[i].assign((size_t)n_cap * n_ch * 4096u, 128u);
        e->st[i].assign(n_cap, K0DcState{0, 0, 0});
    }
    e->sums.assign((size_t)n_cap * max_blk, K0S2{0x5A5A5A5A, 0x5A5A5A5A});
    e->dc_tab.assign((size_t)n_cap * max_blk, 0xDEADBEEFu);
    e->agc_tab.assign((size_t)n_cap * max_blk, (uint16_t)0xBEEFu);
    return e;
}
void wm_emu_chafc_free(void *p) { delete (ChEmu *)p; }
unsigned wm_emu_chafc_pick_tile(uint32_t L, uint32_t M, uint32_t T) { return k0_pick_tile(L, M, T); }
unsigned wm_emu_chafc_convert_tile(uint32_t fmt) { return WM_K0_THREADS * WM_K0_CONV_UNROLL * (16u / k0_bps((int)fmt)); }

/* One push of raw_bytes (multiple of 4096) of EVERY capture: raw = [n_cap][raw_stride]; plan = [n_cap x n_ch] {step, base}, what
 * k0_afc_plan left for this push.  windows = [n_cap x n_ch][window_stride], row v receives the remainder of earlier pushes of pipeline
 * stream v followed by this push's bytes.  Returns the bytes the pipeline would take per stream; *clipped: the push's clip count, all
 * streams. */
long wm_emu_chafc_push(void *p, const uint8_t *raw, size_t raw_stride, size_t raw_bytes, const uint32_t *plan, uint8_t *windows, size_t window_stride,
                       size_t window_cap, uint32_t *clipped)
{
    ChEmu *e = (ChEmu *)p;
    const uint32_t n_in = (uint32_t)(raw_bytes / k0_bps((int)e->fmt)), nv = e->n_cap * e->n_ch;
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
    if (e->R) {                                                  /* per capture, once: not per channel */
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
#define CALL(F) run_ch_gain<F>(e, g)
                BY_FORMAT(e->fmt, CALL)
#undef CALL
            }
    }
    std::vector<K0AfcPush> push(nv);
    for (uint32_t v = 0; v < nv; v++) push[v] = K0AfcPush{plan[2u * v], plan[2u * v + 1u]};

    K0Args a{};
    a.raw = raw; a.raw_stride = raw_stride; a.out = windows; a.out_stride = window_stride; a.taps = e->taps.data();
    a.hist_in = e->hist[e->cur].data(); a.hist_out = e->hist[e->cur ^ 1u].data();
    a.rem_in = e->rem_buf[e->cur].data(); a.rem_out = e->rem_buf[e->cur ^ 1u].data();
    a.n_first = e->n_out; a.in_first = e->n_in; a.n_in = n_in; a.n_out = n_out;
    a.rem_prev = e->rem; a.keep_from = (uint32_t)whole;
    a.L = e->L; a.M = e->M; a.T = e->T; a.tile = e->tile;
    a.gain_q8 = e->gain; a.clipped = clipped;
    a.step = 0xDEADBEEFu;                                        /* the CH && AF form looks neither at the single shift's step nor at the channels' */
    a.n_ch = e->n_ch;
    for (uint32_t c = 0; c < WM_K0_MAX_CH; c++) a.steps[c] = 0xDEADBEEFu;
    a.shift_tab = e->tab.data();
    a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.agc_tab = e->agc ? e->agc_tab.data() : nullptr; a.dc_stride = e->blk_stride;
    a.afc = push.data();
    std::vector<uint32_t> lds((e->resample ? k0_lds_bytes(e->L, e->M, e->T, e->tile) : 4u) / 4u + 1u);
    gridDim = {(n_out + e->tile - 1u) / e->tile, nv, 1};
    for (uint32_t v = 0; v < nv; v++)
        for (uint32_t b = 0; b < gridDim.x; b++) {
            blockIdx = {b, v, 0};
            std::fill(lds.begin(), lds.end(), 0xDEADBEEFu);      /* what a block finds in LDS is not defined */
#define CALL(F) run_ch_stage<F>(e, a, lds.data())
            BY_FORMAT(e->fmt, CALL)
#undef CALL
        }
    e->n_in += n_in; e->n_out = out_end; e->rem = (uint32_t)(total - whole); e->cur ^= 1u;
    return (long)whole;
}

}
