/* spectrum_emu.cpp -- TEST INFRASTRUCTURE: the channel survey of K0 (device source wm_k0_spectrum.h: k0_spectrum_block<FMT, DC>, what
 * k0_spectrum<> runs) on the coroutine block emulator, driven push by push the way wm_api.hip drives the kernel: with a blocker its sums
 * and its plan first (same launch arguments, same double-buffered carried state), then the survey over the push's level blocks, four
 * waves per block, a run of level blocks per wave, into accumulators that live as long as the context.  The 64-bit atomic add and the
 * atomic max the kernel ends with are plain read-modify-writes on the host (wm_k0_spectrum.h: k0_add64 / k0_max32, the pattern of
 * k0_add): the emulator runs one lane at a time. */
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

#include "wm_k0_spectrum.h"

namespace {
struct Emu {
    uint32_t fmt, R, run, cur = 0;
    std::vector<uint32_t> tab;                                   /* [1024] {c, s} */
    K0DcState st[2] = {{0, 0, 0}, {0, 0, 0}};
    std::vector<K0S2> sums;
    std::vector<uint32_t> dc_tab;
    uint64_t sum[WM_K0_SPEC_BINS], blocks;
    uint32_t peak[WM_K0_SPEC_BINS];
};

template <int FMT> void run_sums(const K0DcArgs &d) { block_emu::run_block(WM_K0_THREADS, [&] { k0_dc_sums_block<FMT>(d); }); }
template <int FMT> void run_spec(const Emu *e, const K0SpecArgs &a, int32_t *lds)
{
    if (e->R) block_emu::run_block(64u * WM_K0_SPEC_WAVES, [&] { k0_spectrum_block<FMT, true>(a, lds); });
    else block_emu::run_block(64u * WM_K0_SPEC_WAVES, [&] { k0_spectrum_block<FMT, false>(a, lds); });
}
}

extern "C" {

/* table: what wmbus_shift_design gave (1024 x {c, s}); R: cfg.input_dc (0: no blocker); run: level blocks per wave */
void *wm_emu_spec_new(uint32_t fmt, const int16_t *table, uint32_t R, uint32_t run)
{
    Emu *e = new Emu();
    e->fmt = fmt; e->R = R; e->run = run;
    e->tab.resize(1024u); memcpy(e->tab.data(), table, 4096u);
    memset(e->sum, 0, sizeof e->sum); memset(e->peak, 0, sizeof e->peak); e->blocks = 0;
    return e;
}
void wm_emu_spec_free(void *p) { delete (Emu *)p; }

/* the accumulators as an earlier part of the stream left them */
void wm_emu_spec_preset(void *p, const uint64_t *sum, const uint32_t *peak, uint64_t blocks)
{
    Emu *e = (Emu *)p;
    memcpy(e->sum, sum, sizeof e->sum); memcpy(e->peak, peak, sizeof e->peak); e->blocks = blocks;
}

/* One push of raw_bytes (multiple of 4096) of one capture.  Returns the level blocks of the push. */
long wm_emu_spec_push(void *p, const uint8_t *raw, size_t raw_bytes)
{
    Emu *e = (Emu *)p;
    const uint32_t n_blk = (uint32_t)(raw_bytes / k0_bps((int)e->fmt)) >> WM_K0_DC_LOG2;
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
    a.shift_tab = e->tab.data(); a.sum = e->sum; a.peak = e->peak; a.blocks = &e->blocks;
    a.n_blk = n_blk; a.run = e->run;
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

/* as wmbus_read_spectrum: any pointer may be NULL; reset != 0 zeroes the accumulators behind the read */
long wm_emu_spec_read(void *p, uint64_t *sum, uint32_t *peak, uint64_t *blocks, int reset)
{
    Emu *e = (Emu *)p;
    if (sum) memcpy(sum, e->sum, sizeof e->sum);
    if (peak) memcpy(peak, e->peak, sizeof e->peak);
    if (blocks) *blocks = e->blocks;
    if (reset) { memset(e->sum, 0, sizeof e->sum); memset(e->peak, 0, sizeof e->peak); e->blocks = 0; }
    return (long)WM_K0_SPEC_BINS;
}

}
