/* power_emu.cpp -- TEST INFRASTRUCTURE: channel power (cfg.line_power) on the coroutine block emulator.
 *   wm_emu_pow_*         the band form of the survey kernel (device source wm_k0_spectrum.h: k0_spectrum_block<FMT, DC, AGE, true>, what
 *                        k0_spectrum<FMT, DC, AGE, true> runs) driven push by push the way wm_api.hip drives it: with a blocker its sums and
 *                        its plan first, with ageing k0_spec_age_plan and the fills it asks for, then the kernel over the push's level
 *                        blocks into the accumulators AND into a row of 32 bands per level block.  The 16-lane row sums the kernel makes
 *                        with DPP are xor exchanges here (wm_k0_spectrum.h: k0_row_partner).
 *   wm_emu_pow_channel   the device source of k0_channel_power (wm_k0_power.h: k0_channel_power_block) on the grid wm_api.hip launches.
 *   wm_emu_pow_window    the window helpers the kernel and the host share.
 * The twin of spectrum_emu.cpp and afc_age_emu.cpp. */
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

#include "wm_k0_power.h"

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
    const uint32_t n = 64u * WM_K0_SPEC_WAVES;
    if (e->age) {
        if (e->R) block_emu::run_block(n, [&] { k0_spectrum_block<FMT, true, true, true>(a, lds); });
        else block_emu::run_block(n, [&] { k0_spectrum_block<FMT, false, true, true>(a, lds); });
    } else {
        if (e->R) block_emu::run_block(n, [&] { k0_spectrum_block<FMT, true, false, true>(a, lds); });
        else block_emu::run_block(n, [&] { k0_spectrum_block<FMT, false, false, true>(a, lds); });
    }
}
}

extern "C" {

/* table: what wmbus_shift_design gave (1024 x {c, s}); R: cfg.input_dc (0: no blocker); run: level blocks per wave; age: A (0: the survey
 * never forgets); k_start: the stream's index of the first level block this emulator will see */
void *wm_emu_pow_new(uint32_t fmt, const int16_t *table, uint32_t R, uint32_t run, uint32_t age, uint64_t k_start)
{
    Emu *e = new Emu();
    e->fmt = fmt; e->R = R; e->run = run; e->age = age; e->K = k_start;
    e->tab.resize(1024u); memcpy(e->tab.data(), table, 4096u);
    memset(e->slots, 0, sizeof e->slots);
    return e;
}
void wm_emu_pow_free(void *p) { delete (Emu *)p; }

/* One push of raw_bytes (multiple of 4096) of one capture; rows receives 32 uint32 per level block (poisoned first: a band the kernel does
 * not write shows).  Returns the level blocks of the push. */
long wm_emu_pow_push(void *p, const uint8_t *raw, size_t raw_bytes, uint32_t *rows)
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
    K0SpecArgs a{};
    a.raw = raw; a.raw_stride = 0; a.dc_tab = e->R ? e->dc_tab.data() : nullptr; a.dc_stride = (uint32_t)e->dc_tab.size();
    a.shift_tab = e->tab.data(); a.sum = e->sum(0); a.peak = e->peak(0); a.blocks = e->blocks(0);
    a.n_blk = n_blk; a.run = e->run;
    if (e->age) {
        const K0SpecAgePlan plan = k0_spec_age_plan(e->K, n_blk, e->age);
        for (unsigned s = 0; s < 2u; s++)
            if (plan.clear >> s & 1u) memset(e->slots + s * STRIDE, 0, STRIDE * sizeof(uint64_t));
        a.age = e->age; a.k_first = e->K; a.e_keep = plan.e_keep; a.slot_stride = STRIDE;
    }
    e->K += n_blk;
    std::fill(rows, rows + (size_t)WM_K0_POW_BANDS * n_blk, 0xDEADBEEFu);
    a.bands = rows; a.band_stride = (uint64_t)WM_K0_POW_BANDS * n_blk;
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

/* as wmbus_read_spectrum: the accumulators (with ageing the view, the two slots together) */
long wm_emu_pow_read(void *p, uint64_t *sum, uint32_t *peak, uint64_t *blocks)
{
    Emu *e = (Emu *)p;
    for (unsigned b = 0; b < WM_K0_SPEC_BINS; b++) {
        if (sum) sum[b] = e->sum(0)[b] + e->sum(1)[b];
        if (peak) peak[b] = std::max(e->peak(0)[b], e->peak(1)[b]);
    }
    if (blocks) *blocks = *e->blocks(0) + *e->blocks(1);
    return (long)WM_K0_SPEC_BINS;
}

/* k0_channel_power over one push: rows = [n_cap][n_blk][32]; S = n_cap x n_ch pipeline streams; held = [S] the AFC states' held_hz, or NULL
 * (then centre_hz[n_ch]); P = [2 S][n_blk] (poisoned first). */
void wm_emu_pow_channel(const uint32_t *rows, uint32_t n_cap, uint32_t n_ch, uint32_t n_blk, uint32_t in_hz, const int32_t *centre_hz, const int32_t *chain_hz,
                        const int32_t *held, uint32_t *P)
{
    const uint32_t S = n_cap * n_ch;
    std::vector<K0AfcState> st(S, K0AfcState{0x5A5A5A5A, 0x5Au, 0x5Au, 0x5Au, 0x5Au, {0u, 0u, 0u}});
    if (held) for (uint32_t v = 0; v < S; v++) st[v].held_hz = held[v];
    std::fill(P, P + (size_t)2 * S * n_blk, 0xDEADBEEFu);
    K0PowArgs a{};
    a.bands = rows; a.band_stride = (uint64_t)WM_K0_POW_BANDS * n_blk; a.P = P; a.p_stride = n_blk;
    a.afc = held ? st.data() : nullptr;
    a.S = S; a.n_ch = n_ch; a.n_blk = n_blk; a.in_hz = in_hz;
    for (uint32_t c = 0; c < WM_K0_MAX_CH; c++) a.centre_hz[c] = !held && c < n_ch ? centre_hz[c] : 0x5A5A5A5A;
    a.chain_hz[0] = chain_hz[0]; a.chain_hz[1] = chain_hz[1];
    gridDim = {(n_blk + WM_K0_POW_THREADS / 32u - 1u) / (WM_K0_POW_THREADS / 32u), S, 2};
    for (uint32_t ch = 0; ch < 2u; ch++)
        for (uint32_t v = 0; v < S; v++)
            for (uint32_t b = 0; b < gridDim.x; b++) {
                blockIdx = {b, v, ch};
                block_emu::run_block(WM_K0_POW_THREADS, [&] { k0_channel_power_block(a); });
            }
    blockIdx = {0, 0, 0};
}

/* out = {W, nb, cb, lo, j0} of the window centred on f_hz */
void wm_emu_pow_window(uint32_t in_hz, int64_t f_hz, int64_t *out)
{
    const K0PowWindow w = k0_pow_window(in_hz);
    int64_t cb = 0; uint32_t lo = 0;
    const uint32_t j0 = k0_pow_j0(f_hz, in_hz, w, &cb, &lo);
    out[0] = w.W; out[1] = w.nb; out[2] = cb; out[3] = lo; out[4] = j0;
}

}
