/*
 * wm_api.hip -- host pipeline behind the C ABI of include/wmbus_hip.h.
 *
 * One context owns one HIP stream, the HBM-resident buffers of wm_dev.h, pinned host staging
 * for bursts, and the persistent host packet decoders (4 per capture: chain x framer).
 * There is NO CPU fallback: without a HIP device wmbus_open() fails with WMBUS_ENODEVICE.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include <sys/time.h>

#include "../../include/wmbus_hip.h"
#include "wm_decoder.h"
#include "wm_dev.h"
#include "wm_kernels.hip"
#include "wm_lane_merge.h"
#include "wm_resample_design.h"
#include "wm_spectrum_channels.h"

namespace {

class WorkerPool;              /* wm_host_decode.h */
struct WmLaneRec;              /* wm_launch.h */
thread_local hipStream_t wm_open_on_stream = nullptr;      /* wmbus_batch_open: the context this thread opens next runs on its lane mate's stream */

struct HostDecoder {           /* persistent across pushes */
    wm_decoder dec;
    uint32_t owed;             /* chips to request at the start of the next push */
    uint64_t fed;              /* push in which the decoder last took chips (see the dropped-burst clean-up in wmbus_collect) */
    wmbus_level lev;           /* cfg.line_levels: the level of the burst it is receiving, measured in the push that held its access code */
};

/* Every device and page-locked allocation of a context is made here and recorded; wmbus_close -- and with it every refused open --
 * frees what was recorded, so no buffer can be allocated and not freed.  (Sub-allocations such as Framer::d_sync_seen are views.) */
struct Owned {
    std::vector<void *> dev, pinned;
    hipError_t dbytes(void **p, size_t n) { const hipError_t e = hipMalloc(p, n); if (e == hipSuccess) dev.push_back(*p); return e; }
    template <typename T> hipError_t dalloc(T **p, size_t n) { return dbytes((void **)p, n * sizeof(T)); }
    template <typename T> hipError_t halloc(T **p, size_t n) { const hipError_t e = hipHostMalloc((void **)p, n * sizeof(T)); if (e == hipSuccess) pinned.push_back(*p); return e; }
    void release() { for (void *p : dev) hipFree(p); for (void *p : pinned) hipHostFree(p); dev.clear(); pinned.clear(); }
};

/* One framer's share of a context, indexed by WMBUS_ALGO_*: [0] the run-length framer, [1] clock recovery + time2. */
struct Framer {
    uint32_t C = 0, cap = 0, nseg_cap = 0;             /* segment length (decimated samples), chips a segment's region holds, segments per row at most */
    uint32_t state_bytes = 0;                          /* sizeof(WmRlaState) / sizeof(WmClkState) */
    uint32_t *d_chips = nullptr, *d_counts = nullptr;
    void *d_st_start = nullptr, *d_st_final = nullptr, *d_st_carry = nullptr;   /* carry: [2][rows], see wmbus_ctx.carry_in */
    uint32_t *d_sync_seen = nullptr;                   /* [2][S][nseg_cap] access-code chip seen in region (a view into d_scalars) */
    uint32_t *d_list = nullptr;                        /* re-run list; every verifier has its own: collect's slow path starts from what the LAST verify of each kind left */
    uint32_t *d_bad = nullptr;                         /* [2][nseg_cap][S] the verifier's verdict per segment (K2Args.bad) */
    uint32_t sc = 0;                                   /* SC_* index of its round counters: list round r counts in sc + r, the last verification in sc + rounds */
    unsigned round0 = 0, rounds = 0;                   /* list rounds round0 .. rounds - 1 are enqueued unattended, see WM_MAX_ROUNDS (the run-length framer's start at 1) */
    K2Args k2{};                                       /* this push's launch arguments (collect's slow path re-uses them) */
};

/* The demodulation kernels a context can launch, resolved once in wmbus_open (k1_resolve). */
enum K1Role { K1_FIRST /* first pass without the RSSI */, K1_RSSI /* RSSI of the listed tiles */, K1_FULL /* everything, every tile */,
              K1_REPAIR /* the general kernel: re-run lists, option paths */, K1_ROLES };
struct K1Entry { void (*kernel)(K1Args) = nullptr; uint32_t threads = 0, lds = 0, lds_most = 0; };      /* lds_most: the most any context launches it with (the attribute) */

/* events of a push, on the context's stream (wait_gpu turns pairs of them into wmbus_timing) */
enum { EV_PUSH, EV_K1, EV_K1_END, EV_CLK, EV_RLA, EV_FR_END, EV_K3, EV_K3_END, EV_D2H_END, EV_RS, EV_RS_END /* the RSSI launch over the listed tiles */, EV_COUNT };

}  // namespace

struct wmbus_ctx {
    wmbus_cfg cfg{};
    char err[256] = {0};
    hipStream_t stream = nullptr;                      /* every kernel of the context (inside a batch lane: the lane's stream, wm_batch.h) */
    bool stream_owned = true;                          /* false: the stream is the lane mate's, which closes behind this context */
    WmLaneRec *rec = nullptr;                          /* a batch lane is recording this half of the push: operations are listed, not issued (wm_launch.h) */
    unsigned long long n_single = 0;                   /* kernel launches that left singly (wmbus_batch_lane_stats) */
    hipStream_t copy_stream = nullptr;                 /* wmbus_stage's H2D copies (north_star: "pinned hipMemcpyAsync on a side stream") */
    hipEvent_t ev[EV_COUNT] = {};
    hipEvent_t ev_staged = nullptr;                    /* recorded on copy_stream at process(): the push's input is in HBM */
    hipEvent_t ev_turn = nullptr;                       /* behind the main part of this context's K1: the next context's K1 waits for it */
    uint32_t n_win = 1, fill = 0;                      /* input windows (cfg.input_windows) and the one wmbus_stage fills now */
    /* geometry */
    uint32_t d = 2, S = 1, Mcap = 0, ntiles_cap = 0, T = WM_K1_TILE2, flags = 0;
    /* cfg.input_channels: S = NC x CH is the pipeline's width, pipeline stream v = capture * CH + channel; NC = cfg.n_streams captures own
     * the raw windows and the level tables of K0, everything behind K0 is indexed by v.  Without channels CH = 1 and NC = S. */
    uint32_t NC = 1, CH = 1;
    Framer fr[2];
    Owned mem;
    uint64_t in_stride = 0, n0 = 0;
    size_t push_cap = 0;                               /* bytes of a push the pipeline is sized for: cfg.max_push_bytes, or what that many raw bytes resample to at most */
    /* cfg.input_rate_hz / input_shift_hz / input_dc / input_agc / input_format / input_gain_q8: the stage in front of the demodulation kernel (wm_k0_resample.h) --
     * the resampler (`resample`), which also reads every format, rotates (`shift`) and applies the gain, or for an input at the native
     * rate the conversion kernel alone (L = M = 1, no taps, no history).  wmbus_stage fills the RAW windows; K0
     * writes the window of d_in the pipeline reads.  hist / rem are double-buffered like every carried state (a push reads half
     * `cur`, writes the other).  Every capture advances in lock step, so the counters live here and travel as launch arguments. */
    struct {
        bool on = false, resample = false, shift = false;  /* shift: cfg.input_shift_hz != 0, the rotating instantiations of either kernel */
        bool chan = false;                             /* cfg.input_channels != 0: the channels instantiations (they always rotate) */
        uint32_t steps[WMBUS_MAX_CHANNELS] = {};       /* the phase step of every channel */
        uint32_t fmt = WMBUS_FMT_CU8, bps = 2, gain = 0;   /* cfg.input_format, its raw bytes per sample, cfg.input_gain_q8 */
        uint32_t step = 0;                             /* the shift's phase advance per input sample (k0_shift_design) */
        uint32_t *d_shift_tab = nullptr;               /* [1024] {c, s} int16 */
        /* cfg.input_dc != 0: the I/Q DC blocker -- k0_dc_sums and k0_dc_plan in front of the DC instantiation of either kernel */
        uint32_t dc = 0, dc_stride = 0;                /* R; level blocks (512 input samples) of a full push */
        K0S2 *d_dc_sums = nullptr;                     /* [NC][dc_stride] */
        uint32_t *d_dc_tab = nullptr;                  /* [NC][dc_stride] {dc_I, dc_Q} int16 of the last push's level blocks */
        K0DcState *d_dc_state = nullptr;               /* [2][NC] */
        K0DcArgs dca{};                                /* this push's arguments of the two kernels (k0_plan) */
        /* cfg.input_agc: the per-block AGC -- k0_agc_gain (behind the blocker's two) in front of the AG instantiation of either kernel */
        bool agc = false;
        uint16_t *d_agc_tab = nullptr;                 /* [NC][dc_stride] g of the last push's level blocks */
        K0AgcArgs aga{};                               /* this push's arguments of k0_agc_gain (k0_plan) */
        uint32_t L = 1, M = 1, T = 16, tile = 0, lds = 0, cur = 0, rem = 0;
        uint64_t raw_stride = 0;
        uint8_t *d_raw = nullptr;                      /* [n_win][NC][raw_stride] */
        int16_t *d_taps = nullptr;                     /* [L][T] */
        uint32_t *d_hist = nullptr;                    /* [2][S][T - 1] {I, Q} int16 */
        uint8_t *d_rem = nullptr;                      /* [2][S][4096] */
        uint64_t n_in = 0, n_out = 0;                  /* raw samples pushed / outputs produced so far */
        size_t last_bytes = 0; uint32_t last_win = 0;  /* what the last push handed to the pipeline, and in which window */
        uint32_t last_dc_blocks = 0;                   /* level blocks of the last push (wmbus_read_input_dc, wmbus_read_input_gain) */
        uint64_t last_out = 0;                         /* bytes the last push produced, all captures (wmbus_timing.input_bytes_out) */
        unsigned long long launches = 0;
    } k0;
    /* cfg.input_spectrum: the channel survey (wm_k0_spectrum.h) -- k0_spectrum over the raw bytes of every push, in front of everything else
     * (behind k0_dc_plan where there is a blocker), into accumulators that live as long as the context.  It only reads: a context on the
     * plain cu8 path stays on it.  All nullptr without the option. */
    struct {
        bool on = false;
        uint64_t *d_sum = nullptr;                     /* [NC][512] */
        uint32_t *d_peak = nullptr;                    /* [NC][512] */
        uint64_t *d_blocks = nullptr;                  /* [NC] */
        /* cfg.input_spectrum_age = A: two slots of the three arrays, {sum [NC][512] | blocks [NC] | peak [NC][512]} per slot in ONE
         * allocation (a slot, or both, is cleared with one fill); the pointers above are slot 0's, slot 1's lie slot_stride uint64 behind.
         * K counts the level blocks of the stream: all captures advance in lock step, a reset does not restart it. */
        uint32_t age = 0;
        uint64_t *d_slots = nullptr; uint64_t slot_stride = 0;
        uint64_t K = 0;
    } spec;
    /* cfg.input_afc: automatic frequency correction (wm_k0_afc.h) -- k0_afc_plan behind k0_spectrum and in front of the AFC form of either
     * stage kernel.  The state is double-buffered with k0.cur like every carried state of K0.  All nullptr without the option. */
    struct {
        bool on = false;
        int32_t nominal = 0; uint32_t range = 0, fin = 0;
        /* cfg.input_channel_afc_hz: a lock per channel -- a state and a push entry per pipeline stream v = capture x C + channel, the plan
         * kernel once per v; `n` is the number of states: S with channels, NC without */
        bool chan = false;
        uint32_t ch_range[WMBUS_MAX_CHANNELS] = {};
        uint32_t n = 0;
        K0AfcState *d_state = nullptr;                 /* [2][n] */
        K0AfcPush *d_push = nullptr;                   /* [n] {step, base} of the last push */
        K0AfcArgs args{};                              /* this push's arguments of k0_afc_plan (k0_plan) */
    } afc;
    /* cfg.line_power: channel power (wm_k0_power.h) -- the band form of k0_spectrum writes a row of 32 bands per capture and level block,
     * k0_channel_power (behind k0_afc_plan where there is one) sums every pipeline row's window into P, P travels to pinned host memory
     * with the push, and wait_gpu appends it to the row's history: what decode_host turns into a record per line.  All nullptr / empty
     * without the option. */
    struct {
        bool on = false;
        uint32_t fin = 0, blk_cap = 0, hist = 0;       /* Fin; level blocks of a full push; level blocks kept in front of the current push */
        uint32_t *d_bands = nullptr;                   /* [NC][32 blk_cap] */
        uint32_t *d_P = nullptr, *h_P = nullptr;       /* [2 S][blk_cap] */
        uint64_t K = 0;                                /* the stream's index of the next push's first level block */
        uint64_t last_first = 0; uint32_t last_blk = 0;    /* the push in flight (or the last one): its first level block, their number */
        K0PowArgs args{};                              /* this push's arguments of k0_channel_power */
        std::vector<std::vector<uint32_t>> ring;       /* [2 S] P of level blocks ring_first ...: the history and the last collected push */
        uint64_t ring_first = 0;
        uint64_t got_first = 0; uint32_t got_blk = 0;  /* the last collected push */
    } pw;
    std::vector<wmbus_power> powers;                   /* parallel to `lines` */
    /* cfg.channel_activity: the census of bursts (wm_k0_activity.h) -- k0_activity, behind k0_channel_power, walks every row's complete
     * epochs and leaves this push's records in an arena in ticket order; the ticket count travels with the push, wait_gpu fetches that many
     * records, sorts them by (row, first_block) and keeps them for wmbus_activity.  The tickets are never reset: `taken` is the count in
     * front of the push in flight.  All nullptr / empty without the option. */
    struct {
        bool on = false;
        uint32_t T = 0, H = 0, cap = 0, taken = 0;
        bool launched = false;                         /* the push in flight ran the kernel */
        K0ActState *d_state = nullptr;                 /* [2 S] */
        K0ActRecord *d_arena = nullptr;                /* [cap] */
        uint32_t *d_count = nullptr, *h_count = nullptr;
        std::vector<K0ActRecord> raw;
        std::vector<wmbus_burst> bursts;               /* what the last collect delivered */
    } act;
    /* device buffers */
    uint8_t *d_in = nullptr;                           /* [n_win][S][in_stride] */
    uint8_t *d_hist = nullptr;                         /* [S][4096] the input history of the next push (see k_copy_hist) */
    float *d_dphi = nullptr; uint8_t *d_rssi = nullptr; uint32_t *d_bits = nullptr;
    float *d_lut = nullptr;
    float *d_ema_head = nullptr, *d_ema_tail = nullptr, *d_ema_carry = nullptr;   /* carry: [2][rows], see carry_in */
    /* Carried state is double-buffered: a push reads the exact end state of the previous one from half `carry_in` and
     * commits its own into the other half.  The commits are enqueued before the host knows whether every hand-off was
     * certified; if wmbus_collect has to finish rounds, the re-runs of first tiles / segments still find the state
     * they must start from, and the commit is simply made again. */
    uint32_t carry_in = 0; bool committed = false;
    uint32_t *d_list_ema = nullptr;                     /* RSSI repair list (one entry per row at most) */
    uint32_t *d_scalars = nullptr;                      /* head of ONE allocation zeroed once per push: scalars | sync_seen[0] | sync_seen[1] |
                                                           nchain + bump counter (separate fills cost a context's chain of launches 40 us each) */
    size_t zero_words = 0;
    uint32_t *d_spill = nullptr, *d_chain = nullptr, *d_nchain = nullptr; uint32_t spill_words = 0;   /* WmSpill (wm_dev.h) */
    unsigned ema_rounds = 1;                            /* RSSI hand-off rounds enqueued unattended, see WM_MAX_ROUNDS (the framers': Framer::rounds) */
    bool opt_rounds = true;                             /* hand-off rounds are enqueued unattended (cfg.rounds_on_host = 0) */
    bool poisoned = false, gpu_decode = true;                              /* an internal error left the carried state undefined */
    uint32_t *d_first_bad = nullptr;                    /* [2][S] first uncertified EMA tile of a row, or ~0 */
    /* RSSI on demand (wm_k1_demod.h): the first pass leaves the RSSI out, k3_spans lists the tiles whose RSSI is read, an
     * RS = 2 launch computes those.  Off for contexts with debug taps (they show every sample's RSSI) and for the option
     * kernels; cfg.rssi_full turns it off for A/Bs. */
    bool rs_od = false, rs_full_now = false;            /* rs_full_now: this push has fallen back to the full pass */
    bool rs_this = false;                               /* this push runs on demand (a context whose bursts cover most of its tiles takes the full pass for a while) */
    unsigned rs_pause = 0;                              /* pushes left before on demand is tried again */
    bool k1_big = false;                                /* the first pass without the RSSI runs on 2000-sample tiles of 512 threads (decimation 2, no -s) */
    uint32_t k1_tpb = 1;                                /* tiles per block of the first pass without the RSSI (cfg.k1_tiles_per_block) */
    unsigned clk_form = 4;                              /* cfg.clock_waves: 4 systolic (wm_k2_clock_sys.h), 1 rounds 1-5's one wave per lane group (wm_k2_clock.h) */
    uint32_t k1_tail_pm = 60;                           /* per mille of a push's tiles behind the early hand-over of the K1 turn (enqueue_front_impl) */
    uint32_t *d_rs_flags = nullptr, *d_rs_list = nullptr;   /* [ntiles_cap][S] chains read per (tile, capture); the tiles listed */
    WmItemRec *d_plans = nullptr;                          /* [4 S + hits_cap] what k3_spans leaves k3_bursts about every item */
    uint32_t *d_ckpt = nullptr; uint32_t nck = 0;       /* clock kernel checkpoints [2][S][nseg_cap][nck][16] */
    uint2 *d_hits = nullptr; uint32_t hits_cap = 0;
    uint32_t *d_pending = nullptr;
    uint32_t hdr_cap = 0, words_cap = 0, pkts_cap = 0, bytes_cap = 0;
    /* host (pinned).  The burst kernel writes its results straight into h_hdr / h_words / h_pkts / h_bytes (zero-copy over
     * PCIe: ~1 MB per push once the bursts are decoded on the GPU), so no copy has to wait for a size. */
    uint32_t *h_scalars = nullptr;
    WmBurstHdr *h_hdr = nullptr; uint32_t *h_words = nullptr; uint32_t *h_pending = nullptr;
    WmPkt *h_pkts = nullptr; uint8_t *h_bytes = nullptr;
    void *dv_hdr = nullptr, *dv_words = nullptr, *dv_pkts = nullptr, *dv_bytes = nullptr;    /* their device views */
    uint32_t n_hdr = 0, n_words = 0, n_pkts = 0;
    /* cfg.line_levels (wm_k3_levels.h): the soft-symbol tail [2][2 S][WM_LEV_TAIL], double-buffered with carry_in like every carried state, and
     * the level records k3_levels writes beside h_pkts / h_hdr (pinned, zero-copy like those).  All nullptr without the option. */
    bool lev_on = false;
    float *d_lev_tail = nullptr;
    uint2 *d_lev_src_pkts = nullptr, *d_lev_src_hdr = nullptr;   /* [pkts_cap], [hdr_cap]: where k3_bursts tells k3_levels each record's access-code sample and row */
    WmLevel *h_lev_pkts = nullptr, *h_lev_hdr = nullptr;
    void *dv_lev_pkts = nullptr, *dv_lev_hdr = nullptr;
    std::vector<wmbus_level> levels;                    /* parallel to `lines` */
    /* cfg.crc_repair (wm_k3_repair.h): the repair records k3_repair writes beside h_pkts (pinned, zero-copy like those); it switches
     * lev_on on.  nullptr without the option. */
    bool rep_on = false;
    WmRepair *h_rep_pkts = nullptr;
    void *dv_rep_pkts = nullptr;
    std::vector<wmbus_repair> repairs;                  /* parallel to `lines` */
    /* cfg.s1_rescue (wm_k3_rescue.h): the rescue records k3_rescue writes beside h_rep_pkts, pinned and zero-copy like those; it switches
     * lev_on on.  nullptr without the option. */
    bool res_on = false;
    WmRescue *h_res_pkts = nullptr;
    void *dv_res_pkts = nullptr;
    std::vector<wmbus_rescue> rescues;                  /* parallel to `lines` */
    unsigned res_subjects = 0, res_rescued = 0;         /* of the last collect: subjects a decoder took, and those of them that gave a line */
    /* cfg.line_quality (wm_k3_quality.h): the quality records k3_quality writes beside h_rep_pkts, pinned and zero-copy like those; it
     * switches lev_on on.  nullptr without the option. */
    bool q_on = false;
    WmQuality *h_q_pkts = nullptr;
    void *dv_q_pkts = nullptr;
    std::vector<wmbus_quality> qualities;               /* parallel to `lines` */
    K1Entry k1[K1_ROLES];                               /* the demodulation kernels of this context */
    K1Args k1a{}; uint32_t ntiles = 0;                  /* this push's launch arguments (collect's slow path re-uses them) */
    std::vector<HostDecoder> decs;                      /* [stream][chain][algo] */
    std::vector<wm_twin> twins;                         /* [stream][chain][2]: the last lines printed (cfg.dedup_twins) */
    std::unique_ptr<WorkerPool> pool;                   /* packet-decoder workers, created on first use */
    std::vector<wmbus_line> lines; std::string text;
    WmPush last{}; bool have_last = false, in_flight = false;
    uint64_t push_seq = 0;                              /* pushes enqueued so far */
    /* A push is enqueued in two parts: FRONT (input history, K1, hand-off rounds, both framers, carried state) and BACK
     * (the chips half-received telegrams are owed, K3, the scalars).  Only the back needs what the host packet decoders
     * left behind, so a caller that pipelines (wmbus_batch) enqueues the next push's front BEFORE it decodes the previous
     * one on the host: 2 ms less in every context's chain of dependent work.  wmbus_process = front + back. */
    bool back_due = false, enqueued = false;            /* front enqueued, back not yet; something of this push reached the stream */
    struct timeval arrival{};                           /* wall clock when the push was handed over (its last byte had arrived) */
    /* what wait_gpu() found, kept apart from `last` & co. because the next push's front may be enqueued before decode_host() */
    struct { uint32_t n_hdr = 0, n_pkts = 0; uint64_t m_end = 0, seq = 0; struct timeval arrival{}; bool valid = false; } done;
    std::atomic<uint32_t> short_burst{0};               /* set by the decoder threads of one collect: 1 + header index */
    wmbus_timing tim{};
};

namespace {

int fail(wmbus_ctx *c, int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(c->err, sizeof c->err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return fail((c), WMBUS_EDEVICE, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

#include "wm_launch.h"

/* Hand-off verification runs a few rounds WITHOUT asking the host: verify -> re-run list on the device -> list launch
 * with a fixed grid -> verify ..., each round with its own counter; the host only looks at the last counters when it
 * collects the push and finishes the (rare) leftovers round by round. */
enum { WM_MAX_DEVICES = 64 };                    /* per-device tables (K1 order, kernel attributes); wmbus_open refuses ordinals beyond */
/* How many: wmbus_ctx.ema_rounds / Framer::rounds.  A batch of whole waves enqueues one RSSI round and two framer rounds (bench
 * workload: clock re-runs 1400, then < 10, then 0; run-length 2300, then 0; a third costs every push 0.2 ms of empty launches).
 * A small batch is bound by its chain of dependent launches and by every host round trip in it, and its short segments
 * (wmbus_open) cascade further: it enqueues more rounds, so that the host-driven path (0.5 ms per round) stays the exception. */
enum { WM_MAX_ROUNDS = 6 };                      /* counters per kind of round: rounds + 1 <= 8 slots of the SC_* layout below (the run-length framer's
                                                    index runs to its rounds <= WM_MAX_ROUNDS + 1) */
/* bounded grids of the burst kernels and of the RSSI launch over the listed tiles (launch_k3) */
#ifndef WM_K3_BLOCKS
#define WM_K3_BLOCKS 64           /* build-time A/B (tools/build_variant.sh): r02 256 -> 64 blocks + 6 %, 16 blocks - 9 % */
#endif
enum { WM_RS_BLOCKS = 2048 };
enum { WM_K1_TPB_DEFAULT = 2 };                /* tiles per block of the demodulation kernel's first pass (RSSI on demand), see enqueue_front_impl */
enum { SC_ERR = 0, SC_NHITS = 1, SC_NHDR = 2, SC_NWORDS = 3, SC_NPKTS = 4, SC_NBYTES = 5, SC_SLOW = 6, SC_CHIPS = 8 /* [algo][chain] */,
       SC_RS_N = 12 /* tiles listed for the RSSI-on-demand launch */, SC_RS_FAIL = 13 /* a lane that is read could not prove its value */,
       SC_CLIP = 14 /* K0: output bytes the clamp changed (wmbus_timing.input_clipped) */,
       SC_EMA = 16 /* [ema_rounds + 1] */, SC_CLK = 24 /* [fr[1].rounds + 1] */, SC_RLA = 32 /* [fr[0].rounds + 1] */, SC_COUNT = 40 };
static_assert(WM_MAX_ROUNDS + 2 <= 8 && SC_RLA + WM_MAX_ROUNDS + 2 <= SC_COUNT, "every kind of round keeps its counters inside its eight SC_* slots");

/* 4096 bytes per capture from src + row * sstride + soff to dst + row * dstride (256 threads x 16 bytes).  The input
 * history: the last 4096 staged bytes of a push are put aside (d_hist) when the push is enqueued and placed in front of
 * the window the next push is staged into when THAT push is enqueued -- in between the window stays as it was, so
 * that wmbus_collect's slow path can still re-run the first tile of a capture. */
__global__ void k_copy_hist(const uint8_t *src, uint64_t sstride, uint64_t soff, uint8_t *dst, uint64_t dstride)
{
    const uint4 v = *(const uint4 *)(src + (uint64_t)blockIdx.x * sstride + soff + 16u * threadIdx.x);
    *(uint4 *)(dst + (uint64_t)blockIdx.x * dstride + 16u * threadIdx.x) = v;
}

__global__ void k_copy_word(uint32_t *dst, uint32_t v) { *dst = v; }
__global__ void k_and_word(uint32_t *dst, uint32_t v) { *dst &= v; }

__global__ void k_fill(uint8_t *p, uint64_t stride, uint32_t n, uint8_t v)
{
    uint8_t *row = p + (uint64_t)blockIdx.x * stride;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) row[i] = v;
}

__global__ void k_carry(const uint32_t *fin, uint32_t *carry, uint32_t words, uint32_t rows, uint32_t nseg_cap, uint32_t nseg)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    for (uint32_t k = 0; k < words; k++) carry[(uint64_t)r * words + k] = fin[((uint64_t)r * nseg_cap + nseg - 1) * words + k];
}

/* wmbus_timing.chips: chips produced per (framer, chain) in this push = sum of the settled segment counts.  One
 * atomic per wave and sum (82 000 threads adding to four words directly cost the whole GPU 15 % while they ran). */
__global__ __launch_bounds__(256) void k_sum_counts(WmPush g, const uint32_t *counts0, const uint32_t *counts1, uint32_t *sums)
{
    const uint32_t n0 = 2u * g.nseg_cap[0] * g.S, n1 = 2u * g.nseg_cap[1] * g.S;
    uint32_t part[4] = {0u, 0u, 0u, 0u};
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n0 + n1; t += gridDim.x * blockDim.x) {
        const uint32_t algo = t >= n0, i = algo ? t - n0 : t;
        const uint32_t seg = i % g.nseg_cap[algo], ch = i / g.nseg_cap[algo] / g.S;
        if (seg < g.nseg[algo] && (g.flags & (algo ? WM_F_T2A : WM_F_RLA))) part[algo * 2u + ch] += (algo ? counts1 : counts0)[i];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t v = part[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63u) == 0u && v) atomicAdd(sums + k, v);
    }
}

/* the reference's default switches: what the demodulation kernel without the option paths (k1_demod2<.., GEN = false>) and RSSI on demand are built for */
bool default_switches(uint32_t flags)
{
    return (flags & (WM_F_ACCURATE | WM_F_T1C1 | WM_F_S1 | WM_F_APPROX1 | WM_F_APPROX2)) == (WM_F_ACCURATE | WM_F_T1C1 | WM_F_S1);
}

template <int D, bool SHIFT, bool GEN, bool FAST = false, int RS = 0, int NT = 256> K1Entry k1_entry(const wmbus_ctx *c)
{
    return K1Entry{k1_demod2<D, SHIFT, GEN, FAST, RS, NT>, (uint32_t)NT, (uint32_t)K1GeoT<NT>::smem(D ? D : (int)c->d, SHIFT), (uint32_t)K1GeoT<NT>::smem(D ? D : (int)WM_MAX_DECIM, SHIFT)};
}

/* The kernel of every role for decimation D (0: any rate without a kernel of its own) with or without -s.  Tolerance mode is an option
 * of the default switches' kernels only (everything else stays exact; the listed tiles' RSSI is the same in tolerance mode). */
template <int D, bool SHIFT> void k1_resolve_for(wmbus_ctx *c)
{
    const bool tol = c->cfg.tolerance_mode;
    c->k1[K1_REPAIR] = k1_entry<D, SHIFT, true>(c);
    c->k1[K1_FULL] = D == 0 || !default_switches(c->flags) ? c->k1[K1_REPAIR] : tol ? k1_entry<D, SHIFT, false, true>(c) : k1_entry<D, SHIFT, false>(c);
    if (!c->rs_od) return;                       /* RSSI on demand (open_geometry has checked the switches): the first pass without it ... */
    c->k1[K1_FIRST] = tol ? k1_entry<D, SHIFT, false, true, 1>(c) : k1_entry<D, SHIFT, false, false, 1>(c);
    if (c->k1_big)                               /* ... on the 2000-sample tile of 512 threads (the launch's grid counts THOSE tiles; wmbus_ctx.k1_big) */
        c->k1[K1_FIRST] = tol ? k1_entry<2, false, false, true, 1, 512>(c) : k1_entry<2, false, false, false, 1, 512>(c);
    c->k1[K1_RSSI] = k1_entry<D, SHIFT, false, false, 2>(c);
}

/* wmbus_open: one entry per role this context can launch, each kernel's dynamic LDS allowed for */
int k1_resolve(wmbus_ctx *c)
{
    const bool sh = c->flags & WM_F_SHIFT;
    if (c->cfg.prefilter == WMBUS_PREFILTER_POLYPHASE)
        for (auto &e : c->k1) e = K1Entry{k1_demod_ppf, 256u, (uint32_t)K1PpfGeo::smem(), (uint32_t)K1PpfGeo::smem()};
    else switch (c->d) {
    case 2: sh ? k1_resolve_for<2, true>(c) : k1_resolve_for<2, false>(c); break;
    case 3: sh ? k1_resolve_for<3, true>(c) : k1_resolve_for<3, false>(c); break;
    case 4: sh ? k1_resolve_for<4, true>(c) : k1_resolve_for<4, false>(c); break;
    case 5: sh ? k1_resolve_for<5, true>(c) : k1_resolve_for<5, false>(c); break;
    default: sh ? k1_resolve_for<0, true>(c) : k1_resolve_for<0, false>(c); break;      /* any other rate */
    }
    for (const auto &e : c->k1)
        if (e.kernel) HIPCHK(c, hipFuncSetAttribute((const void *)e.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.lds_most));
    return 0;
}

int launch_k1(wmbus_ctx *c, K1Role role, const K1Args &a, dim3 grid)
{
    const K1Entry &e = c->k1[role];
    wm_launch(c, e.kernel, grid, dim3(e.threads), e.lds, a);
    HIPCHK(c, hipGetLastError());
    return 0;
}

/* The kernels' arithmetic (table-driven atan2 included) on arbitrary operand pairs. */
__global__ void k_selftest(const float *a, const float *b, float *o_sqrt, float *o_div, float *o_atan2, float *o_disc, uint32_t n)
{
    __shared__ float tab[WM_ATAN_TAB_WORDS];
    for (int k = threadIdx.x; k < WM_ATAN_TAB_WORDS; k += blockDim.x) wm_atan_tab_word(k, tab);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    o_sqrt[i] = wm_sqrt_dom(fabsf(a[i]));
    o_div[i] = wm_div_dom(a[i], b[i]);
    o_atan2[i] = wm_atan2f_tab(a[i], b[i], tab);
    o_disc[i] = wm_discriminator_tab(a[i], b[i], b[(i + 1) % n], a[(i + 1) % n], tab);
}

/* The demodulation kernel's two low-pass filters (k1_fir_t / k1_fir_s, the very functions its stage B inlines) over one row of
 * arbitrary floats: x[0 .. n + 48) with the 48 samples of history in front, n a multiple of 4 up to 976 (one tile of the kernel); out[0 .. n) the 11-tap
 * filter, out[n .. 2n) the 46-tap one.  For the operands a capture cannot easily produce: signed zeros above all (a soft symbol
 * must never be -0, the clock kernel takes the slicer's bit from its sign). */
__global__ void __launch_bounds__(256) k_selftest_fir(const float *x, float *out, uint32_t n)
{
    __shared__ __attribute__((aligned(16))) float row[K1Geo::YD];
    for (uint32_t w = threadIdx.x; w < (uint32_t)K1Geo::YD; w += blockDim.x) row[w] = w >= 4u && w - 4u < n + 48u ? x[w - 4u] : 0.0f;
    __syncthreads();
    K1Args a{};
    a.g.S = 1; a.g.Mcap = n; a.dphi = out;
    k1_fir_t<false>(a, row, (int)threadIdx.x, 0, 0, (int)n);
    k1_fir_s<false>(a, row, (int)threadIdx.x, 0, 0, (int)n);
}

/* The run-length framer's divisions (wm_udiv / wm_sdiv of wm_k2_rla.h, the very functions its edge loop inlines) against the
 * compiler's integer division and the definition of a truncated quotient (q b <= ua < q b + b).  res[0] = wrong results,
 * res[1..2] = cases looked at (64 bit), res[4 + 2 i], res[5 + 2 i] = the operands (dividend, divisor) of the i-th wrong one, i < 16.
 * Part 0, the reciprocal path over its whole domain: blockIdx.x + 4 = b in 4..4095, every multiple q b below 2^24 and its two
 * neighbours, with either sign through wm_sdiv.  Part 1, the bounds: blockIdx.x + 1 = b in 1..8192, ua in 2^24 - 64 .. 2^24 + 64
 * (above 2^24 - 1 and for b outside 4..4095 the integer divide must be taken: the reciprocal's estimate is not within 1 there)
 * and ua in 0..128, either sign where the dividend fits wm_sdiv. */
__global__ void __launch_bounds__(256) k_selftest_udiv(uint32_t *res, const uint32_t part)
{
    uint32_t looked = 0;
    auto check = [&](const uint32_t ua, const uint32_t b) {
        const uint32_t q = wm_udiv(ua, b);
        bool ok = q == ua / b && (uint64_t)q * b <= ua && ua - (uint64_t)q * b < b;
        if (ua < (1u << 31)) {
            const int a = -(int)ua;
            ok = ok && wm_sdiv(a, (int)b) == a / (int)b && wm_sdiv((int)ua, (int)b) == (int)ua / (int)b;
        }
        looked++;
        if (!ok) {
            const uint32_t i = atomicAdd(&res[0], 1u);
            if (i < 16u) { res[4u + 2u * i] = ua; res[5u + 2u * i] = b; }
        }
    };
    const uint32_t t = blockIdx.y * blockDim.x + threadIdx.x, nt = gridDim.y * blockDim.x;
    if (part == 0u) {
        const uint32_t b = blockIdx.x + 4u;
        for (uint32_t q = t; q <= ((1u << 24) - 1u) / b + 1u; q += nt) {
            const uint32_t m = q * b;                        /* at most 2^24 + 4094 */
            if (m >= 1u && m - 1u < (1u << 24)) check(m - 1u, b);
            if (m < (1u << 24)) check(m, b);
            if (m + 1u < (1u << 24)) check(m + 1u, b);
        }
    } else {
        const uint32_t b = blockIdx.x + 1u;
        for (uint32_t i = t; i < 129u + 129u; i += nt) check(i < 129u ? (1u << 24) - 64u + i : i - 129u, b);
    }
    atomicAdd((unsigned long long *)(res + 2), (unsigned long long)looked);
}

/* The demodulation kernels of one device's contexts run ONE AFTER THE OTHER (each fills the GPU on its own -- VALU
 * bound -- so two of them side by side only time-slice, while one of them beside the other contexts' latency- and
 * memory-bound framer kernels is complementary).  The order is kept on the GPU: a context's K1 waits for the event
 * behind the K1 launched before it, so no host thread sits in the way (a host-side turn held across the launches of
 * everything behind K1 made the turn 2.9 ms longer than the kernel). */
struct K1Chain { std::mutex m; hipEvent_t last = nullptr; const wmbus_ctx *owner = nullptr; };
K1Chain k1_chain[WM_MAX_DEVICES];

/* A context's turn in that chain: taken in front of its K1 launches, handed on behind them.  Outside a batch lane the chain's
 * mutex is held across the launches, for the life of this object.  A lane RECORDS the push (wm_launch.h), so the turn is
 * taken and handed on by two recorded operations, when the launches are issued and not when they are listed; the lane's
 * merge keeps the operations between them together (wm_lane_merge.h).  wm_turn_held: the chain this thread holds between
 * those two operations -- the lane lets go of it if an operation in between fails. */
thread_local K1Chain *wm_turn_held = nullptr;
struct K1Turn {
    wmbus_ctx *const c; K1Chain &kc; bool locked = false;
    K1Turn(wmbus_ctx *c_, K1Chain &kc_) : c(c_), kc(kc_) {}
    ~K1Turn() { if (locked) kc.m.unlock(); }
    int take()
    {
        wmbus_ctx *const cc = c; K1Chain *const k = &kc;
        if (!c->rec) {
            kc.m.lock(); locked = true;
            if (kc.last && kc.owner != c) HIPCHK(c, hipStreamWaitEvent(c->stream, kc.last, 0));
            return 0;
        }
        return wm_op(c, "taking the K1 turn", [=]() -> hipError_t {
            if (wm_turn_held) return hipErrorInvalidValue;          /* the merge never interleaves two turns */
            k->m.lock(); wm_turn_held = k;
            return k->last && k->owner != cc ? hipStreamWaitEvent(cc->stream, k->last, 0) : hipSuccess;
        });
    }
    int hand_on(hipEvent_t ev)
    {
        wmbus_ctx *const cc = c; K1Chain *const k = &kc;
        if (!c->rec) { kc.last = ev; kc.owner = c; return 0; }
        return wm_op(c, "handing on the K1 turn", [=]() -> hipError_t {
            if (wm_turn_held != k) return hipErrorInvalidValue;
            k->last = ev; k->owner = cc;
            wm_turn_held = nullptr; k->m.unlock();
            return hipSuccess;
        });
    }
};

/* One HIP stream per receiver context (two with cfg.input_windows = 2); ROCm maps streams onto GPU_MAX_HW_QUEUES hardware
 * queues (4 by default) round robin, and streams that share a queue serialise against each other: eight contexts on four
 * queues run at 81 instead of 143 Gsamples/s, ten on eight at 107 (r03 A/B).  (That, and not the hosts' CPU quota, is also the
 * 100-110 Gsamples/s of rounds 7-18: their hosts preset four queues, and a caller's setting wins.  Since round 19 a batch with
 * fewer queues than contexts drives neighbouring contexts as one lane on one stream, with paired launches -- wm_batch.h -- and
 * runs at the rate of a queue per context: 174 against 102)  The runtime reads the variable when it
 * initialises (the first HIP call of the process), so wmbus_runtime_init() (include/wmbus_hip.h) must run before that:
 * wmbus_batch_open calls it, the CLI calls it first thing, an embedder that uses HIP itself calls it (or sets the
 * variable) before its own first HIP call -- a caller's own setting wins.  (Rounds 2-3 did this in a load-time constructor:
 * a setenv behind the host application's back)  16 covers the default batch (8 contexts, 12 in tolerance mode) with and without copy streams; with 16
 * queues and 8 contexts the rate is the one with 8 queues.  (bench.py and INTEGRATION.md used to ask the caller for this.) */
double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

static void power_record(wmbus_power *out, const K0PowRecord &r)
{
    out->first_block = r.first_block; out->signal = r.signal; out->noise = r.noise; out->ratio_q8 = r.ratio_q8; out->n_signal = r.n_signal; out->n_noise = r.n_noise;
}

#include "wm_host_decode.h"

extern "C" {

void wmbus_runtime_init(void)
{
    /* setenv is not safe against concurrent getenv: call this before the process starts threads that read the
     * environment (the CLI: first statement of main) */
    if (!getenv("WMBUS_KEEP_HW_QUEUES")) setenv("GPU_MAX_HW_QUEUES", "16", 0);
}

void wmbus_default_cfg(wmbus_cfg *cfg)
{
    memset(cfg, 0, sizeof *cfg);
    cfg->decimation = 2; cfg->accurate_atan = 1; cfg->t1c1_enabled = 1; cfg->s1_enabled = 1;
    cfg->rla_enabled = 1; cfg->time2_enabled = 1; cfg->n_streams = 1;
    cfg->max_push_bytes = 4u << 20;
}

int wmbus_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int wmbus_resampler_design(unsigned in_hz, unsigned out_hz, unsigned *L, unsigned *M, unsigned *T, int16_t *taps, size_t cap)
{
    return k0_design(in_hz, out_hz, L, M, T, taps, cap) ? WMBUS_EINVAL : WMBUS_OK;
}

int wmbus_shift_design(unsigned in_hz, int shift_hz, uint32_t *step, int16_t *table, size_t cap)
{
    return k0_shift_design(in_hz, shift_hz, step, table, cap) ? WMBUS_EINVAL : WMBUS_OK;
}

long wmbus_read_input_dc(wmbus_ctx *c, unsigned stream, int16_t *iq, size_t cap_pairs)
{
    if (!c || stream >= c->NC || !iq) return WMBUS_EINVAL;
    if (!c->k0.dc) return fail(c, WMBUS_EINVAL, "read_input_dc: the context was opened without cfg.input_dc");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_input_dc: collect the push first");
    const size_t n = std::min(cap_pairs, (size_t)c->k0.last_dc_blocks);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n) HIPCHK(c, hipMemcpy(iq, c->k0.d_dc_tab + (size_t)stream * c->k0.dc_stride, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return (long)n;
}

long wmbus_read_input_gain(wmbus_ctx *c, unsigned stream, uint16_t *g, size_t cap)
{
    if (!c || stream >= c->NC || !g) return WMBUS_EINVAL;
    if (!c->k0.agc) return fail(c, WMBUS_EINVAL, "read_input_gain: the context was opened without cfg.input_agc");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_input_gain: collect the push first");
    const size_t n = std::min(cap, (size_t)c->k0.last_dc_blocks);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n) HIPCHK(c, hipMemcpy(g, c->k0.d_agc_tab + (size_t)stream * c->k0.dc_stride, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return (long)n;
}

long wmbus_read_spectrum(wmbus_ctx *c, unsigned stream, uint64_t *sum, uint32_t *peak, uint64_t *blocks, int reset)
{
    if (!c || stream >= c->NC) return WMBUS_EINVAL;
    if (!c->spec.on) return fail(c, WMBUS_EINVAL, "read_spectrum: the context was opened without cfg.input_spectrum");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_spectrum: collect the push first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    uint64_t *d_sum = c->spec.d_sum + (size_t)stream * WM_K0_SPEC_BINS, *d_blocks = c->spec.d_blocks + stream;
    uint32_t *d_peak = c->spec.d_peak + (size_t)stream * WM_K0_SPEC_BINS;
    if (c->spec.age) {                                       /* the view: the two slots together (SPECTRUM AGE); a reset clears both */
        const uint64_t st = c->spec.slot_stride;
        uint64_t h_sum[2][WM_K0_SPEC_BINS], h_blocks[2];
        uint32_t h_peak[2][WM_K0_SPEC_BINS];
        for (unsigned sl = 0; sl < 2u; sl++) {
            HIPCHK(c, hipMemcpyAsync(h_sum[sl], d_sum + sl * st, sizeof h_sum[sl], hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_peak[sl], d_peak + 2u * sl * st, sizeof h_peak[sl], hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&h_blocks[sl], d_blocks + sl * st, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
            if (reset) {
                HIPCHK(c, hipMemsetAsync(d_sum + sl * st, 0, WM_K0_SPEC_BINS * sizeof(uint64_t), c->stream));
                HIPCHK(c, hipMemsetAsync(d_peak + 2u * sl * st, 0, WM_K0_SPEC_BINS * sizeof(uint32_t), c->stream));
                HIPCHK(c, hipMemsetAsync(d_blocks + sl * st, 0, sizeof(uint64_t), c->stream));
            }
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (unsigned b = 0; b < WM_K0_SPEC_BINS; b++) {
            if (sum) sum[b] = h_sum[0][b] + h_sum[1][b];
            if (peak) peak[b] = std::max(h_peak[0][b], h_peak[1][b]);
        }
        if (blocks) *blocks = h_blocks[0] + h_blocks[1];
        return (long)WM_K0_SPEC_BINS;
    }
    /* on the context's own stream, which is idle behind a collect (a synchronous copy would bring the NULL stream's queue in: open_init) */
    if (sum) HIPCHK(c, hipMemcpyAsync(sum, d_sum, WM_K0_SPEC_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (peak) HIPCHK(c, hipMemcpyAsync(peak, d_peak, WM_K0_SPEC_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (blocks) HIPCHK(c, hipMemcpyAsync(blocks, d_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (reset) {
        HIPCHK(c, hipMemsetAsync(d_sum, 0, WM_K0_SPEC_BINS * sizeof(uint64_t), c->stream));
        HIPCHK(c, hipMemsetAsync(d_peak, 0, WM_K0_SPEC_BINS * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(d_blocks, 0, sizeof(uint64_t), c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return (long)WM_K0_SPEC_BINS;
}

long wmbus_read_input_afc(wmbus_ctx *c, unsigned stream, wmbus_afc *out)
{
    if (!c || stream >= (c->afc.chan ? c->S : c->NC) || !out) return WMBUS_EINVAL;      /* with a lock per channel `stream` is the pipeline stream */
    if (!c->afc.on) return fail(c, WMBUS_EINVAL, "read_input_afc: the context was opened without cfg.input_afc");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_input_afc: collect the push first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    K0AfcState st{};                                         /* half k0.cur: what the last push committed (before the first push: the initial state) */
    HIPCHK(c, hipMemcpyAsync(&st, c->afc.d_state + (size_t)c->k0.cur * c->afc.n + stream, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = wmbus_afc{st.held_hz, st.locked, st.changes, st.ratio_q8};
    return 0;
}

int wmbus_spectrum_channels(unsigned in_hz, const uint64_t *sum, const uint32_t *peak, uint64_t blocks, unsigned width_hz, unsigned min_ratio_q8,
                            unsigned rel, wmbus_channel_hit *out, unsigned cap)
{
    return k0_spectrum_channels(in_hz, sum, peak, blocks, width_hz, min_ratio_q8, rel, out, cap);
}

unsigned long long wmbus_resampler_launches(const wmbus_ctx *ctx) { return ctx ? ctx->k0.launches : 0ull; }

const char *wmbus_last_error(const wmbus_ctx *ctx) { return ctx ? ctx->err : "null context"; }

void wmbus_close(wmbus_ctx *c)
{
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    /* an open that was refused before it had a stream (bad device ordinal, bad geometry: the caller closes the handle it reads
     * the message from) never took part in the K1 order, and its cfg.device may lie outside the table */
    if (c->stream && c->cfg.device >= 0 && c->cfg.device < WM_MAX_DEVICES) {
        K1Chain &kc = k1_chain[c->cfg.device];
        std::lock_guard<std::mutex> lk(kc.m);
        if (kc.owner == c) { kc.last = nullptr; kc.owner = nullptr; }      /* nobody may wait on an event that is about to go */
    }
    c->mem.release();
    for (auto &e : c->ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : {c->ev_staged, c->ev_turn}) if (e) hipEventDestroy(e);
    if (c->copy_stream && c->copy_stream != c->stream) { hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); }
    if (c->stream && c->stream_owned) hipStreamDestroy(c->stream);
    delete c;
}

/* wmbus_open, step 1: is the configuration one the library takes, and is its device there?  Designs the resampler on the way (a rate
 * without a design is a refusal; `k0_taps` keeps its taps for open_init) and the phase step of cfg.input_shift_hz. */
static int open_validate(wmbus_ctx *c, std::vector<int16_t> &k0_taps)
{
    const wmbus_cfg *cfg = &c->cfg;
    if (cfg->decimation < 1 || cfg->decimation > WM_MAX_DECIM) return fail(c, WMBUS_EINVAL, "decimation must be 1..%u", WM_MAX_DECIM);
    if (cfg->n_streams < 1) return fail(c, WMBUS_EINVAL, "n_streams must be >= 1");
    if (cfg->max_push_bytes < WMBUS_BLOCK_BYTES || cfg->max_push_bytes % WMBUS_BLOCK_BYTES)
        return fail(c, WMBUS_EINVAL, "max_push_bytes must be a positive multiple of 4096");
    if (cfg->prefilter != WMBUS_PREFILTER_BOXCAR && cfg->prefilter != WMBUS_PREFILTER_POLYPHASE)
        return fail(c, WMBUS_EINVAL, "prefilter must be WMBUS_PREFILTER_BOXCAR or WMBUS_PREFILTER_POLYPHASE");
    if (cfg->atan_mode < WMBUS_ATAN_LIBM || cfg->atan_mode > WMBUS_ATAN_APPROX2)
        return fail(c, WMBUS_EINVAL, "atan_mode must be WMBUS_ATAN_LIBM, WMBUS_ATAN_APPROX1 or WMBUS_ATAN_APPROX2");
    if (cfg->prefilter == WMBUS_PREFILTER_POLYPHASE && (cfg->decimation != 2 || cfg->simultaneous))
        return fail(c, WMBUS_EINVAL, "the polyphase pre-filter is the 1.6 MS/s design of rtl_wmbus.c:258-294: decimation 2, no -s");
    if (cfg->input_format > WMBUS_FMT_CF32) return fail(c, WMBUS_EINVAL, "input_format must be WMBUS_FMT_CU8, _CS8, _CS16 or _CF32 (got %u)", cfg->input_format);
    if (cfg->input_gain_q8 > 65535u) return fail(c, WMBUS_EINVAL, "input_gain_q8 must be 1 ... 65535 (x 1/256 ... x 256; 0: x 1), got %u", cfg->input_gain_q8);
    if (cfg->input_dc > WM_K0_DC_MAX_R) return fail(c, WMBUS_EINVAL, "input_dc must be 0 (off) or 1 ... %u (time constant 2^input_dc x 512 input samples), got %u", WM_K0_DC_MAX_R, cfg->input_dc);
    if (cfg->input_agc > 1u) return fail(c, WMBUS_EINVAL, "input_agc must be 0 (off) or 1, got %u", cfg->input_agc);
    if (cfg->input_agc && cfg->input_gain_q8 != 0u && cfg->input_gain_q8 != 256u)
        return fail(c, WMBUS_EINVAL, "input_agc takes the place of input_gain_q8: leave that 0 or 256 (got %u)", cfg->input_gain_q8);
    if (cfg->line_levels > 1u) return fail(c, WMBUS_EINVAL, "line_levels must be 0 or 1, got %u", cfg->line_levels);
    if (cfg->line_power > 1u) return fail(c, WMBUS_EINVAL, "line_power must be 0 or 1, got %u", cfg->line_power);
    if (cfg->channel_activity > 1u) return fail(c, WMBUS_EINVAL, "channel_activity must be 0 or 1, got %u", cfg->channel_activity);
    if (cfg->channel_activity_ratio_q8 && !cfg->channel_activity)
        return fail(c, WMBUS_EINVAL, "channel_activity_ratio_q8 = %u without channel_activity", cfg->channel_activity_ratio_q8);
    if (cfg->channel_activity_ratio_q8 && (cfg->channel_activity_ratio_q8 < 257u || cfg->channel_activity_ratio_q8 > 65535u))
        return fail(c, WMBUS_EINVAL, "channel_activity_ratio_q8 must be 0 or 257 ... 65535, got %u", cfg->channel_activity_ratio_q8);
    c->act.on = cfg->channel_activity != 0u;
    c->act.T = cfg->channel_activity_ratio_q8 ? cfg->channel_activity_ratio_q8 : WM_K0_ACT_RATIO_Q8;
    c->pw.on = cfg->line_power != 0u || c->act.on;                    /* the census reads the timeline of CHANNEL POWER */
    if (cfg->crc_repair > 1u) return fail(c, WMBUS_EINVAL, "crc_repair must be 0 or 1, got %u", cfg->crc_repair);
    if (cfg->crc_repair && cfg->bursts_to_host)
        return fail(c, WMBUS_EINVAL, "crc_repair works on the telegrams the GPU decodes: with bursts_to_host there is nothing it could repair");
    c->rep_on = cfg->crc_repair != 0u;
    /* a power record needs its line's access-code sample: the level record carries it; the repair reads that sample and the soft-symbol tail */
    if (cfg->line_quality > 1u) return fail(c, WMBUS_EINVAL, "line_quality must be 0 or 1, got %u", cfg->line_quality);
    if (cfg->line_quality && cfg->bursts_to_host)
        return fail(c, WMBUS_EINVAL, "line_quality works on the telegrams the GPU decodes: with bursts_to_host there is nothing it could measure");
    c->q_on = cfg->line_quality != 0u;                                /* k3_quality reads each packet's access-code sample: k3_bursts leaves it for the level stage */
    if (cfg->s1_rescue > 1u) return fail(c, WMBUS_EINVAL, "s1_rescue must be 0 or 1, got %u", cfg->s1_rescue);
    if (cfg->s1_rescue && cfg->bursts_to_host)
        return fail(c, WMBUS_EINVAL, "s1_rescue works on the telegrams the GPU decodes: with bursts_to_host there is nothing it could rescue");
    if (cfg->s1_rescue && (!cfg->s1_enabled || !cfg->time2_enabled))
        return fail(c, WMBUS_EINVAL, "s1_rescue works on S1 telegrams of the time2 framer: with %s = 0 there is nothing it could rescue", !cfg->s1_enabled ? "s1_enabled" : "time2_enabled");
    c->res_on = cfg->s1_rescue != 0u;                                 /* k3_rescue finds a packet's chips from its access-code sample, as k3_repair does */
    c->lev_on = cfg->line_levels != 0u || c->pw.on || c->rep_on || c->q_on || c->res_on;
    if (cfg->input_spectrum > 1u) return fail(c, WMBUS_EINVAL, "input_spectrum must be 0 or 1, got %u", cfg->input_spectrum);
    c->spec.on = cfg->input_spectrum != 0u || c->pw.on;          /* the band rows are the survey's */
    auto &k = c->k0;
    k.dc = cfg->input_dc; k.agc = cfg->input_agc != 0u;
    k.fmt = cfg->input_format; k.bps = k0_bps((int)cfg->input_format); k.gain = cfg->input_gain_q8;
    static_assert(WMBUS_MAX_CHANNELS == WM_K0_MAX_CH, "K0Args.steps holds a step per channel");
    if (cfg->input_channels > WMBUS_MAX_CHANNELS) return fail(c, WMBUS_EINVAL, "input_channels must be 0 (off) or 1 ... %d, got %u", WMBUS_MAX_CHANNELS, cfg->input_channels);
    if (cfg->input_channels && cfg->input_shift_hz)
        return fail(c, WMBUS_EINVAL, "input_shift_hz must be 0 with input_channels: every channel has its own shift in input_channel_hz (got input_shift_hz = %d)", cfg->input_shift_hz);
    for (unsigned ch = 0; ch < cfg->input_channels; ch++) {
        const unsigned fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
        const char *why = k0_shift_design(fin, cfg->input_channel_hz[ch], &k.steps[ch], nullptr, 0);
        if (why) return fail(c, WMBUS_EINVAL, "%s (input_channel_hz[%u] = %d, limit +-%u at the input rate %u)", why, ch, cfg->input_channel_hz[ch], fin / 2u, fin);
        k.chan = true;
    }
    if (cfg->input_shift_hz) {
        const unsigned fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
        const char *why = k0_shift_design(fin, cfg->input_shift_hz, &k.step, nullptr, 0);
        if (why) return fail(c, WMBUS_EINVAL, "%s (input_shift_hz = %d, limit +-%u at the input rate %u)", why, cfg->input_shift_hz, fin / 2u, fin);
        k.shift = true;
    }
    if (cfg->input_afc > 1u) return fail(c, WMBUS_EINVAL, "input_afc must be 0 (off) or 1, got %u", cfg->input_afc);
    if (cfg->input_afc_range_hz && !cfg->input_afc) return fail(c, WMBUS_EINVAL, "input_afc_range_hz = %u without input_afc", cfg->input_afc_range_hz);
    if (cfg->input_afc) {
        if (cfg->input_channels) return fail(c, WMBUS_EINVAL, "input_afc together with input_channels: AFC finds one offset per capture, not one per channel");
        auto &f = c->afc;
        f.fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
        f.nominal = cfg->input_shift_hz; f.range = cfg->input_afc_range_hz ? cfg->input_afc_range_hz : WM_K0_AFC_RANGE_HZ;
        const int64_t reach = (int64_t)(f.nominal < 0 ? -(int64_t)f.nominal : (int64_t)f.nominal) + (int64_t)f.range;
        if (f.fin < 800000u || 2 * reach > (int64_t)f.fin)
            return fail(c, WMBUS_EINVAL, "input_afc: |input_shift_hz| + input_afc_range_hz = %lld lies beyond half the input rate %u", (long long)reach, f.fin);
        f.on = true; c->spec.on = true;                          /* the survey is AFC's measurement */
        k.shift = false;                                         /* the AFC form rotates, with a step of its own per capture and push */
    }
    for (unsigned ch = 0; ch < WMBUS_MAX_CHANNELS; ch++) {       /* a lock per channel: any non-zero entry is the switch */
        const unsigned range = cfg->input_channel_afc_hz[ch];
        if (!range) continue;
        if (ch >= cfg->input_channels)
            return fail(c, WMBUS_EINVAL, "input_channel_afc_hz[%u] = %u without that channel (input_channels = %u)", ch, range, cfg->input_channels);
        if (cfg->input_afc) return fail(c, WMBUS_EINVAL, "input_channel_afc_hz together with input_afc: the array is the switch of a channel list");
        auto &f = c->afc;
        f.fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
        const int64_t hz = cfg->input_channel_hz[ch], reach = (hz < 0 ? -hz : hz) + (int64_t)range;
        if (f.fin < 800000u || 2 * reach > (int64_t)f.fin)
            return fail(c, WMBUS_EINVAL, "input_channel_afc_hz: |input_channel_hz[%u]| + input_channel_afc_hz[%u] = %lld lies beyond half the input rate %u", ch, ch, (long long)reach, f.fin);
        f.ch_range[ch] = range;
        f.on = true; f.chan = true; c->spec.on = true;           /* the survey is AFC's measurement */
    }
    if (cfg->input_spectrum_age > 31u) return fail(c, WMBUS_EINVAL, "input_spectrum_age must be 0 (the survey never forgets) or 1 ... 31 (epochs of 2^A level blocks), got %u", cfg->input_spectrum_age);
    if (cfg->input_spectrum_age && !c->spec.on) return fail(c, WMBUS_EINVAL, "input_spectrum_age = %u without a survey: set input_spectrum or input_afc", cfg->input_spectrum_age);
    c->spec.age = cfg->input_spectrum_age;
    if (cfg->input_rate_hz && cfg->input_rate_hz != cfg->decimation * 800000u) {
        unsigned L = 0, M = 0, T = 0;
        k0_taps.resize((size_t)WM_K0_MAX_L * WM_K0_MAX_T);
        const char *why = k0_design(cfg->input_rate_hz, cfg->decimation * 800000u, &L, &M, &T, k0_taps.data(), k0_taps.size());
        if (why) return fail(c, WMBUS_EINVAL, "%s (input_rate_hz = %u, output rate %u)", why, cfg->input_rate_hz, cfg->decimation * 800000u);
        if (k.fmt == WMBUS_FMT_CS16 || k.fmt == WMBUS_FMT_CF32 || k.shift || k.chan || c->afc.on)
            for (unsigned p = 0; p < L; p++) {                   /* 16-bit samples (a shifted cu8 / cs8 sample is one): |acc| <= 32768 sum|taps| must stay inside the kernel's int32 */
                int64_t abs_total = 0;
                for (unsigned t = 0; t < T; t++) abs_total += std::abs((int)k0_taps[(size_t)p * T + t]);
                if (32768ll * abs_total >= (1ll << 31)) return fail(c, WMBUS_EINVAL, "input_rate_hz: the resampler's accumulator bound for 16-bit input is exceeded (phase %u)", p);
            }
        k.on = true; k.resample = true; k.L = L; k.M = M; k.T = T;
        k.tile = k0_pick_tile(L, M, T);
        if (!k.tile) return fail(c, WMBUS_EINVAL, "input_rate_hz: the resampler's tile does not fit the LDS (L = %u, M = %u, T = %u)", L, M, T);
        k.lds = k0_lds_bytes(L, M, T, k.tile);
    } else if (cfg->input_format != WMBUS_FMT_CU8 || (cfg->input_gain_q8 != 0u && cfg->input_gain_q8 != 256u) || k.shift || k.dc || k.agc || k.chan || c->afc.on) {
        /* the native rate in another format, with a gain, with a shift, with the DC blocker, with the AGC, with channels or with AFC: the conversion kernel alone */
        k.on = true; k.L = k.M = k.T = 1u;
        k.tile = WM_K0_THREADS * WM_K0_CONV_UNROLL * (16u / k.bps); k.lds = 0u;
    }
    if (cfg->device < 0 || cfg->device >= WM_MAX_DEVICES) return fail(c, WMBUS_EINVAL, "device must be 0..%d", WM_MAX_DEVICES - 1);
    if (wmbus_device_count() <= cfg->device) return fail(c, WMBUS_ENODEVICE, "no HIP device %d (this library has no CPU fallback)", cfg->device);
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(c, WMBUS_EDEVICE, "hipSetDevice(%d) failed", cfg->device);
    return WMBUS_OK;
}

/* step 2: every size, count and switch of the context from its configuration -- arithmetic only, no HIP call */
static int open_geometry(wmbus_ctx *c)
{
    const wmbus_cfg *cfg = &c->cfg;
    Framer &rla = c->fr[WMBUS_ALGO_RLA], &clk = c->fr[WMBUS_ALGO_T2A];
    c->d = cfg->decimation;
    c->NC = cfg->n_streams; c->CH = cfg->input_channels ? cfg->input_channels : 1u;
    if ((uint64_t)c->NC * c->CH > 0x7FFFFFFFull / 4u)            /* 4 S decoder rows and 2 S x segments lanes are counted in 32 bits */
        return fail(c, WMBUS_EINVAL, "n_streams x input_channels = %u x %u is more pipeline streams than a context takes", c->NC, c->CH);
    c->S = c->NC * c->CH;                                    /* the pipeline's width: every default below that goes by batch width takes it */
    c->n_win = cfg->input_windows == 2 ? 2u : 1u;
    /* the pipeline behind K0 is sized for what a full raw push resamples (converts) to, plus the remainder in front of it */
    c->push_cap = cfg->max_push_bytes;
    if (c->k0.on) {
        const uint64_t most = ((uint64_t)(cfg->max_push_bytes / c->k0.bps) * c->k0.L + c->k0.M - 1u) / c->k0.M * 2u;
        c->push_cap = (size_t)((most + WMBUS_BLOCK_BYTES - 1u) / WMBUS_BLOCK_BYTES * WMBUS_BLOCK_BYTES + WMBUS_BLOCK_BYTES);
        c->k0.raw_stride = (cfg->max_push_bytes + 255u) / 256u * 256u;
        c->k0.dc_stride = (uint32_t)(cfg->max_push_bytes / c->k0.bps) >> WM_K0_DC_LOG2;
    }
    if (c->pw.on) {
        auto &w = c->pw;
        w.fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
        w.blk_cap = (uint32_t)(cfg->max_push_bytes / c->k0.bps) >> WM_K0_DC_LOG2;
        /* Nn + G + ceil(0.15 Fin / 512) level blocks in front of the current push: the noise window of the longest telegram that ends in it */
        w.hist = (w.fin + 25599u) / 25600u + (w.fin + 51199u) / 51200u + (uint32_t)((3ull * w.fin + 10239u) / 10240u);
        if (c->act.on) { c->act.H = k0_act_epochs(w.fin); c->act.cap = 2u * c->S * k0_act_row_cap(w.blk_cap); }
    }
    /* Time segments: 32768 / 8192 decimated samples for batches of whole waves (r02 / r03 A/Bs: clock 65536 -8 %, 16384 -25 %;
     * run-length 16384 -9 %, 4096 -20 %).  A batch with fewer captures than a wave has lanes is bound by how long ONE lane
     * walks (5 us per 32 samples whatever runs beside it), not by the work: its segments shrink with the capture count, down
     * to 8192 / 2048 for a single capture (one 2^22-sample push of one capture: 29 -> 9 ms; the result does not depend on the
     * segmentation, test_result_independent_of_segmentation). */
    uint32_t k = 1;
    while (k < 8u && c->S * k < 64u) k *= 2u;              /* 1 for >= 64 captures ... 8 for fewer than 16 */
    c->clk_form = cfg->clock_waves == 1u ? 1u : 4u;
    if (c->clk_form != 4u)
        clk.C = 32768u / std::min(k, 4u);              /* one capture, r04: 9.3 / 8.8 / 7.7 ms per configs[1] push with 4096 / 8192 / 16384, 9.5 / 9.0 / 10.5 for configs[2]: 8192 */
    else
        /* the systolic form walks a segment in 0.4 of the time (round 6, one capture of configs[1]: 5.6 / 4.9 / 4.25 / 5.8 ms per push with
         * 8192 / 16384 / 32768 / 65536, against 7.6 with the one-wave form's 8192): 32768 whatever the batch size -- and 65536 where the
         * demodulation kernel is the heavier side (exact arithmetic, 1.6 MS/s, no -s: the warm-ups of 12288 / 24576 samples are a quarter
         * less work per sample; bench workload 181-187 against 174-181 Gsamples/s, tolerance mode 199 against 202, configs[2] 161 against 171) */
        clk.C = c->S >= 64u && !cfg->tolerance_mode && cfg->decimation == 2u && !cfg->simultaneous ? 65536u : 32768u;
    /* a live stream's pushes are short (the CLI's 1 MiB = 2^18 decimated samples at 1.6 MS/s): a push of two to eight 32768-sample
     * segments is as long as its one lane with a full warm-up, 57 344 samples; with 16384 that lane is 40 960 (one capture, ms per push of
     * 2^17 / 2^18 / 2^19 input samples: 5.1 / 4.6 / 3.9 -> 2.8 / 3.4 / 3.4; 2^22: 4.3 against 4.8, so long pushes keep 32768) */
    const uint64_t mp = c->push_cap / 2u / std::max(1u, cfg->decimation);      /* a push's decimated samples at most */
    if (c->clk_form == 4u && c->S < 64u && mp > 32768u && mp <= (1u << 19)) clk.C = 16384u;      /* <= 32768: one segment from its exact start */
    if (cfg->seg_len) clk.C = cfg->seg_len;
    /* run-length segments: 4096 (r04 A/B on the bench workload: 151.0 / 151.1 against 148.9 / 150.6 with round 3's 8192 and
     * 136.3 / 134.1 with 2048); 2048 with -s, where S1 telegrams -- 30-100 ms, several segments long -- are expected in both
     * chains and every segment inside one is re-run in a chain walk whose length is the telegram's whatever the segment
     * length, while first pass and first list round scale with it (configs[2] batch: 92.8 / 110.3 / 133.3 Gsamples/s with
     * 8192 / 4096 / 2048, 124.9 with 1024) */
    rla.C = cfg->rla_seg_len ? cfg->rla_seg_len : std::max(2048u, (cfg->simultaneous ? 2048u : 4096u) / k);
    for (const Framer &f : c->fr)
        if (f.C < 1024u || f.C > (1u << 20) || (f.C & (f.C - 1)))
            return fail(c, WMBUS_EINVAL, "seg_len / rla_seg_len must be powers of two in [1024, 1048576]");
    c->cfg.warmup_t1c1 = cfg->warmup_t1c1 ? (cfg->warmup_t1c1 + 31u) & ~31u : 12288u;   /* whole 32-sample blocks */
    c->cfg.warmup_s1 = cfg->warmup_s1 ? (cfg->warmup_s1 + 31u) & ~31u : 24576u;
    c->cfg.rla_lookback = cfg->rla_lookback ? (cfg->rla_lookback + 31u) & ~31u : 1024u;
    c->flags = (cfg->atan_mode == WMBUS_ATAN_APPROX1 ? WM_F_APPROX1 : cfg->atan_mode == WMBUS_ATAN_APPROX2 ? WM_F_APPROX2 : 0) |
               (cfg->simultaneous ? WM_F_SHIFT : 0) | (cfg->accurate_atan ? WM_F_ACCURATE : 0) | (cfg->remove_dc ? WM_F_DC : 0) |
               (cfg->t1c1_enabled ? WM_F_T1C1 : 0) | (cfg->s1_enabled ? WM_F_S1 : 0) | (cfg->rla_enabled ? WM_F_RLA : 0) |
               (cfg->time2_enabled ? WM_F_T2A : 0);
    c->ema_rounds = c->S < 64u ? 2 : 1;
    clk.sc = SC_CLK; clk.round0 = 0; clk.rounds = c->S < 64u ? 5 : 2;
    c->opt_rounds = !cfg->rounds_on_host;
    /* the run-length framer gets as many list rounds as the clock kernel (round 3: one fewer -- enough for 1.6 MS/s captures,
     * "2300 re-runs, then 0", but configs[2] (-d 5 -s) leaves 750 lanes after the first round and fell to the host-driven
     * path on EVERY push: 64 ms per step instead of 25); its counters start at index 1 (its list rounds: 1 .. rounds - 1) */
    rla.sc = SC_RLA; rla.round0 = 1; rla.rounds = std::min<unsigned>(clk.rounds + 1u, WM_MAX_ROUNDS + 1u);
    /* ... and one more with -s: S1 telegrams (30-100 ms) lie in BOTH chains' bands there, a telegram is a chain of twenty to forty
     * run-length segments that only a walk from its first one settles, and two list rounds left a remainder in every tenth push of
     * configs[2] (round 5: rla_round = 10 994, 5 088, then the host-driven path; an empty round costs 0.2 ms) */
    if (cfg->simultaneous) rla.rounds = std::min<unsigned>(rla.rounds + 1u, WM_MAX_ROUNDS + 1u);
    c->T = (uint32_t)WM_K1_TILE2;
    c->ntiles_cap = (uint32_t)((c->push_cap / 2 / c->d + 1 + 8 + c->T - 1) / c->T);
    c->Mcap = (c->ntiles_cap * c->T + 255) / 256 * 256;     /* whole tiles (partial tiles still store full runs); slicer-word rows 32-byte aligned */
    for (Framer &f : c->fr) f.nseg_cap = (c->Mcap + f.C - 1) / f.C;
    rla.state_bytes = sizeof(WmRlaState); clk.state_bytes = sizeof(WmClkState);
    clk.cap = clk.C / 4 + 8;       /* time2: the lock logic needs >= 4 samples per chip */
    /* run-length: a primary region of half a chip per sample (four times the nominal eight samples per chip); the
     * reference's bit-length tracker has no floor -- switch combinations (-d 3 -s -o -a on a capture with both modes)
     * and interferers drag it to a third of a sample per chip for a while (3.1 chips per sample seen, found by the host
     * emulation campaigns), and exact silence ends in one long run -- such segments continue in the spill arena
     * (WmSpill, wm_dev.h); a push never fails for want of chip storage */
    rla.cap = (rla.C / 2 + 8 + 7) / 8 * 8;
    /* K1 stages whole tiles: the partial last tile of a push reads up to (tile + halo) x d input samples past the
     * staged bytes (never used: they only feed outputs beyond M) -- the row must hold them */
    c->in_stride = (WM_HIST_BYTES + c->push_cap + 2ull * (WM_K1_TILE2 + WM_K1_HALO + 16) * WM_MAX_DECIM + WM_IN_SLACK + 255) / 256 * 256;
    c->rs_od = !cfg->rssi_full && !cfg->keep_taps && cfg->prefilter != WMBUS_PREFILTER_POLYPHASE && c->d >= 2 && c->d <= 5 && default_switches(c->flags);
    /* the larger tile of the first pass: decimation 2 without -s (the LDS of a 512-thread block at d >= 3 or with the -s staging
     * would cost more occupancy than the halo saves) */
    c->k1_big = c->rs_od && c->d == 2 && !(c->flags & WM_F_SHIFT) && !cfg->k1_small_tile;
    c->k1_tail_pm = cfg->tolerance_mode ? 0u : 60u;
    c->k1_tpb = cfg->k1_tiles_per_block ? std::min(cfg->k1_tiles_per_block, 64u) : WM_K1_TPB_DEFAULT;
    const uint64_t dec_total = (uint64_t)c->S * c->Mcap, want = cfg->spill_words ? cfg->spill_words : std::max<uint64_t>(1u << 20, dec_total / 16);
    c->spill_words = (uint32_t)std::min<uint64_t>((want + WM_SPILL_CHUNK - 1) / WM_SPILL_CHUNK * WM_SPILL_CHUNK, 0xFFFF0000u);
    c->nck = clk.C / WM_CK_SAMPLES ? clk.C / WM_CK_SAMPLES - 1 : 0;
    c->hdr_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(65536, dec_total / 1024), 1u << 24);
    c->hits_cap = c->hdr_cap;
    /* bursts that still travel as chips are the ones whose plan reaches past the end of the push (every such hit is
     * shipped with the chips up to the end, at most 16 x 290 + 1 of them) and the continuations of those the decoders
     * took: room for two longest bursts per (capture, chain, framer); beyond that bursts are dropped with a warning */
    c->gpu_decode = !cfg->bursts_to_host;                /* else: every burst to the host decoders as chips (A/B, tests) */
    c->words_cap = c->gpu_decode ? (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, 4ull * c->S * 2 * WM_MAXCHIPS_S1), 1u << 28)
                                 : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, dec_total / 8), 1u << 29);
    c->pkts_cap = c->hdr_cap;
    c->bytes_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, dec_total / 64), 1u << 30);
    if (cfg->burst_caps[0]) { c->hdr_cap = cfg->burst_caps[0]; c->hits_cap = std::max(c->hits_cap, c->hdr_cap); }      /* tests: tiny burst storage, to reach the overflow paths */
    if (cfg->burst_caps[1]) c->words_cap = cfg->burst_caps[1];
    if (cfg->burst_caps[2]) c->pkts_cap = cfg->burst_caps[2];
    if (cfg->burst_caps[3]) c->bytes_cap = cfg->burst_caps[3];
    return WMBUS_OK;
}

/* step 3: streams, events, the demodulation kernels and every buffer (recorded in c->mem: wmbus_close frees them) */
static int open_allocate(wmbus_ctx *c)
{
    Owned &m = c->mem;
    const uint64_t rows = 2ull * c->S;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    /* the second context of a batch lane runs on its mate's stream (wm_batch.h): a stream of its own would take a place on a
     * hardware queue, beside some other lane's, for nothing */
    if (wm_open_on_stream) { c->stream = wm_open_on_stream; c->stream_owned = false; }
    else A(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    /* the side stream for wmbus_stage's copies exists where it can overlap something: with two input windows.  (Every
     * stream takes a hardware queue -- ROCm maps streams onto GPU_MAX_HW_QUEUES of them round robin -- and two contexts'
     * compute streams that end up on one queue serialise: an idle copy stream per context halved the 8-context rate.) */
    if (c->n_win == 2) A(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)); else c->copy_stream = c->stream;
    for (auto &ev : c->ev) A(hipEventCreate(&ev));
    A(hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming));
    A(hipEventCreateWithFlags(&c->ev_turn, hipEventDisableTiming));
    A(m.dalloc(&c->d_in, (size_t)c->in_stride * c->S * c->n_win));
    A(m.dalloc(&c->d_hist, (size_t)WM_HIST_BYTES * c->S));
    if (c->k0.on) {
        A(m.dalloc(&c->k0.d_raw, (size_t)c->k0.raw_stride * c->NC * c->n_win));
        if (c->k0.resample) {
            A(m.dalloc(&c->k0.d_taps, (size_t)c->k0.L * c->k0.T));
            A(m.dalloc(&c->k0.d_hist, (size_t)2 * c->S * (c->k0.T - 1u)));
        }
        A(m.dalloc(&c->k0.d_rem, (size_t)2 * c->S * WMBUS_BLOCK_BYTES));
        if (c->k0.dc) {
            A(m.dalloc(&c->k0.d_dc_sums, (size_t)c->NC * c->k0.dc_stride));
            A(m.dalloc(&c->k0.d_dc_tab, (size_t)c->NC * c->k0.dc_stride));
            A(m.dalloc(&c->k0.d_dc_state, (size_t)2 * c->NC));
        }
        if (c->k0.agc) A(m.dalloc(&c->k0.d_agc_tab, (size_t)c->NC * c->k0.dc_stride));
    }
    if (c->k0.shift || c->k0.chan || c->spec.on) A(m.dalloc(&c->k0.d_shift_tab, (size_t)WM_K0_SHIFT_ENTRIES));      /* the survey's window and twiddles are this table's */
    if (c->spec.on && !c->spec.age) {
        A(m.dalloc(&c->spec.d_sum, (size_t)c->NC * WM_K0_SPEC_BINS));
        A(m.dalloc(&c->spec.d_peak, (size_t)c->NC * WM_K0_SPEC_BINS));
        A(m.dalloc(&c->spec.d_blocks, (size_t)c->NC));
    }
    if (c->spec.age) {
        c->spec.slot_stride = (uint64_t)c->NC * (WM_K0_SPEC_BINS + 1u + WM_K0_SPEC_BINS / 2u);
        A(m.dalloc(&c->spec.d_slots, (size_t)2 * c->spec.slot_stride));
        c->spec.d_sum = c->spec.d_slots; c->spec.d_blocks = c->spec.d_sum + (size_t)c->NC * WM_K0_SPEC_BINS;
        c->spec.d_peak = (uint32_t *)(c->spec.d_blocks + c->NC);
    }
    if (c->pw.on) {
        A(m.dalloc(&c->pw.d_bands, (size_t)c->NC * WM_K0_POW_BANDS * c->pw.blk_cap));
        A(m.dalloc(&c->pw.d_P, (size_t)rows * c->pw.blk_cap));
        A(m.halloc(&c->pw.h_P, (size_t)rows * c->pw.blk_cap));
        c->pw.ring.assign((size_t)rows, std::vector<uint32_t>());
    }
    if (c->act.on) {
        A(m.dalloc(&c->act.d_state, (size_t)rows));
        A(m.dalloc(&c->act.d_arena, (size_t)c->act.cap));
        A(m.dalloc(&c->act.d_count, (size_t)1));
        A(m.halloc(&c->act.h_count, (size_t)1));
    }
    if (c->afc.on) {
        c->afc.n = c->afc.chan ? c->S : c->NC;
        A(m.dalloc(&c->afc.d_state, (size_t)2 * c->afc.n));
        A(m.dalloc(&c->afc.d_push, (size_t)c->afc.n));
    }
    A(m.dalloc(&c->d_dphi, (size_t)rows * c->Mcap));
    A(m.dalloc(&c->d_rssi, (size_t)rows * c->Mcap));
    A(m.dalloc(&c->d_bits, (size_t)rows * (c->Mcap / 32)));
    A(m.dalloc(&c->d_lut, (size_t)2 * 32 * WM_MAX_DECIM));
    A(m.dalloc(&c->d_ema_head, (size_t)rows * c->ntiles_cap));
    A(m.dalloc(&c->d_ema_tail, (size_t)rows * c->ntiles_cap));
    A(m.dalloc(&c->d_ema_carry, (size_t)2 * rows));
    A(m.dalloc(&c->d_first_bad, (size_t)rows));
    A(m.dalloc(&c->d_list_ema, (size_t)rows));
    if (c->rs_od) {
        A(m.dalloc(&c->d_rs_flags, (size_t)c->ntiles_cap * c->S));
        A(m.dalloc(&c->d_rs_list, (size_t)c->ntiles_cap * c->S));
        A(m.dalloc(&c->d_plans, (size_t)4 * c->S + c->hits_cap));
    }
    size_t n_seen = 0;
    for (Framer &f : c->fr) {
        const size_t segs = (size_t)rows * f.nseg_cap;
        A(m.dalloc(&f.d_chips, segs * f.cap));
        A(m.dalloc(&f.d_counts, segs));
        A(m.dbytes(&f.d_st_start, segs * f.state_bytes));
        A(m.dbytes(&f.d_st_final, segs * f.state_bytes));
        A(m.dbytes(&f.d_st_carry, (size_t)2 * rows * f.state_bytes));
        A(m.dalloc(&f.d_list, (size_t)rows * (&f == &c->fr[WMBUS_ALGO_T2A] ? std::max(c->fr[0].nseg_cap, c->fr[1].nseg_cap) : f.nseg_cap)));
        A(m.dalloc(&f.d_bad, segs));
        n_seen += segs;
    }
    A(m.dalloc(&c->d_spill, (size_t)c->spill_words));
    A(m.dalloc(&c->d_chain, (size_t)rows * c->fr[0].nseg_cap * WM_SPILL_LEVELS));
    A(m.dalloc(&c->d_ckpt, std::max<size_t>(16, (size_t)rows * c->fr[1].nseg_cap * c->nck * 16)));
    c->zero_words = SC_COUNT + n_seen + (size_t)rows * c->fr[0].nseg_cap + 1;      /* scalars | sync_seen[0] | sync_seen[1] | nchain + bump counter */
    A(m.dalloc(&c->d_scalars, c->zero_words));
    c->fr[0].d_sync_seen = c->d_scalars + SC_COUNT;
    c->fr[1].d_sync_seen = c->fr[0].d_sync_seen + (size_t)rows * c->fr[0].nseg_cap;
    c->d_nchain = c->fr[1].d_sync_seen + (size_t)rows * c->fr[1].nseg_cap;
    A(m.dalloc(&c->d_hits, (size_t)c->hits_cap));
    A(m.dalloc(&c->d_pending, (size_t)4 * c->S));
    A(m.halloc(&c->h_scalars, SC_COUNT));
    A(m.halloc(&c->h_hdr, (size_t)c->hdr_cap));
    A(m.halloc(&c->h_words, (size_t)c->words_cap));
    A(m.halloc(&c->h_pkts, (size_t)c->pkts_cap));
    A(m.halloc(&c->h_bytes, (size_t)c->bytes_cap));
    A(m.halloc(&c->h_pending, (size_t)4 * c->S));
    if (c->lev_on) {
        A(m.dalloc(&c->d_lev_tail, (size_t)2 * rows * WM_LEV_TAIL));
        A(m.dalloc(&c->d_lev_src_pkts, (size_t)c->pkts_cap));
        A(m.dalloc(&c->d_lev_src_hdr, (size_t)c->hdr_cap));
        A(m.halloc(&c->h_lev_pkts, (size_t)c->pkts_cap));
        A(m.halloc(&c->h_lev_hdr, (size_t)c->hdr_cap));
        if (e == hipSuccess) { A(hipHostGetDevicePointer(&c->dv_lev_pkts, c->h_lev_pkts, 0)); A(hipHostGetDevicePointer(&c->dv_lev_hdr, c->h_lev_hdr, 0)); }
    }
    if (c->rep_on) {
        A(m.halloc(&c->h_rep_pkts, (size_t)c->pkts_cap));
        if (e == hipSuccess) A(hipHostGetDevicePointer(&c->dv_rep_pkts, c->h_rep_pkts, 0));
    }
    if (c->res_on) {
        A(m.halloc(&c->h_res_pkts, (size_t)c->pkts_cap));
        if (e == hipSuccess) A(hipHostGetDevicePointer(&c->dv_res_pkts, c->h_res_pkts, 0));
    }
    if (c->q_on) {
        A(m.halloc(&c->h_q_pkts, (size_t)c->pkts_cap));
        if (e == hipSuccess) A(hipHostGetDevicePointer(&c->dv_q_pkts, c->h_q_pkts, 0));
    }
    if (e == hipSuccess) { A(hipHostGetDevicePointer(&c->dv_hdr, c->h_hdr, 0)); A(hipHostGetDevicePointer(&c->dv_words, c->h_words, 0)); }
    if (e == hipSuccess) { A(hipHostGetDevicePointer(&c->dv_pkts, c->h_pkts, 0)); A(hipHostGetDevicePointer(&c->dv_bytes, c->h_bytes, 0)); }
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? WMBUS_ENOMEM : WMBUS_EDEVICE, "allocation failed: %s", hipGetErrorString(e));
    return k1_resolve(c);
}

/* step 4: the state a fresh context carries into its first push = the reference's zero-initialised statics */
static int open_init(wmbus_ctx *c, const std::vector<int16_t> &k0_taps)
{
    const uint64_t rows = 2ull * c->S;
    hipError_t e = hipSuccess;
    auto A = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    /* the verifiers' verdict per segment, for the chain walk of the re-run lanes (K2Args.bad).  Zeroed on the context's own stream: a
     * synchronous hipMemset runs on the NULL stream, whose hardware queue then takes part in the round-robin of streams onto
     * queues -- eight contexts lost 5 % to that in round 4's A/Bs. */
    for (Framer &f : c->fr) A(hipMemsetAsync(f.d_bad, 0, (size_t)rows * f.nseg_cap * sizeof(uint32_t), c->stream));
    if (c->k0.on) A(hipMemsetAsync(c->k0.d_rem, 128, (size_t)2 * c->S * WMBUS_BLOCK_BYTES, c->stream));
    if (c->k0.resample) {                                    /* history before a stream's first sample: x = 0 */
        A(hipMemsetAsync(c->k0.d_hist, 0, (size_t)2 * c->S * (c->k0.T - 1u) * sizeof(uint32_t), c->stream));
        A(hipMemcpyAsync(c->k0.d_taps, k0_taps.data(), (size_t)c->k0.L * c->k0.T * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    }
    if (c->k0.dc) A(hipMemsetAsync(c->k0.d_dc_state, 0, (size_t)2 * c->NC * sizeof(K0DcState), c->stream));      /* started = 0: A[0] = S[0] << R */
    std::vector<int16_t> shift_tab;
    if (c->spec.age) A(hipMemsetAsync(c->spec.d_slots, 0, (size_t)2 * c->spec.slot_stride * sizeof(uint64_t), c->stream));
    else if (c->spec.on) {
        A(hipMemsetAsync(c->spec.d_sum, 0, (size_t)c->NC * WM_K0_SPEC_BINS * sizeof(uint64_t), c->stream));
        A(hipMemsetAsync(c->spec.d_peak, 0, (size_t)c->NC * WM_K0_SPEC_BINS * sizeof(uint32_t), c->stream));
        A(hipMemsetAsync(c->spec.d_blocks, 0, (size_t)c->NC * sizeof(uint64_t), c->stream));
    }
    std::vector<K0AfcState> afc_init;
    if (c->afc.on) {                                         /* unlocked, at the nominal, phase 0: both halves */
        afc_init.assign((size_t)2 * c->afc.n, K0AfcState{c->afc.nominal, 0u, 0u, 0u, 0u, {0u, 0u, 0u}});
        if (c->afc.chan) for (size_t v = 0; v < afc_init.size(); v++) afc_init[v].held_hz = c->cfg.input_channel_hz[v % c->CH];      /* every channel at its own nominal */
        A(hipMemcpyAsync(c->afc.d_state, afc_init.data(), afc_init.size() * sizeof(K0AfcState), hipMemcpyHostToDevice, c->stream));
        A(hipMemsetAsync(c->afc.d_push, 0, (size_t)c->afc.n * sizeof(K0AfcPush), c->stream));
    }
    std::vector<K0ActState> act_init;
    if (c->act.on) {                                         /* no epoch yet: an empty ring, no open run, no ticket taken */
        act_init.assign((size_t)rows, K0ActState{});
        for (K0ActState &s : act_init) std::fill(s.ring, s.ring + 64, WM_K0_ACT_NONE);
        A(hipMemcpyAsync(c->act.d_state, act_init.data(), act_init.size() * sizeof(K0ActState), hipMemcpyHostToDevice, c->stream));
        A(hipMemsetAsync(c->act.d_count, 0, sizeof(uint32_t), c->stream));
        *c->act.h_count = 0u;
    }
    if (c->k0.shift || c->k0.chan || c->spec.on) {           /* {c, s} per entry: the dword the kernels read */
        shift_tab.resize(2u * WM_K0_SHIFT_ENTRIES);
        k0_shift_design(800000u, 0, nullptr, shift_tab.data(), shift_tab.size());
        A(hipMemcpyAsync(c->k0.d_shift_tab, shift_tab.data(), shift_tab.size() * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    }
    A(hipMemsetAsync(c->d_ema_carry, 0, 2 * rows * sizeof(float), c->stream));
    if (c->lev_on) A(hipMemsetAsync(c->d_lev_tail, 0, (size_t)2 * rows * WM_LEV_TAIL * sizeof(float), c->stream));      /* no window reaches in front of the stream: never read */
    /* a disabled chain (-p T / -p S) never writes its hand-off records: they must compare equal, not hold what an
     * earlier context left in the recycled allocation */
    A(hipMemsetAsync(c->d_ema_head, 0, (size_t)rows * c->ntiles_cap * sizeof(float), c->stream));
    A(hipMemsetAsync(c->d_ema_tail, 0, (size_t)rows * c->ntiles_cap * sizeof(float), c->stream));
    A(hipMemsetAsync(c->d_first_bad, 0xFF, rows * sizeof(uint32_t), c->stream));
    A(hipMemsetAsync(c->fr[WMBUS_ALGO_T2A].d_st_carry, 0, 2 * rows * sizeof(WmClkState), c->stream));
    const std::vector<WmRlaState> init(2 * rows, WmRlaState{0, 8 * 256, 0, 0u, 0u, 0u, 24, 24});   /* rtl_wmbus.c:628-637,717-726 */
    A(hipMemcpyAsync(c->fr[WMBUS_ALGO_RLA].d_st_carry, init.data(), 2 * rows * sizeof(WmRlaState), hipMemcpyHostToDevice, c->stream));
    A(hipMemsetAsync(c->d_scalars, 0, c->zero_words * sizeof(uint32_t), c->stream));
    A(hipMemsetAsync(c->d_pending, 0, 4 * c->S * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_fill, dim3(c->S * c->n_win), dim3(256), 0, c->stream, c->d_in, c->in_stride, (uint32_t)c->in_stride, (uint8_t)128);
    hipLaunchKernelGGL(k_fill, dim3(c->S), dim3(256), 0, c->stream, c->d_hist, (uint64_t)WM_HIST_BYTES, (uint32_t)WM_HIST_BYTES, (uint8_t)128);
    /* frequency-translation LUT, built with the host libm exactly like rtl_wmbus.c:974-993 */
    const int fs_khz = (int)c->d * 800;
    std::vector<float> lut(2 * 32 * WM_MAX_DECIM, 0.f);
    for (size_t n = 0; n < (size_t)(fs_khz / 25); n++) {
        const double phi = (2. * M_PI * (25 * (double)n)) / fs_khz;
        lut[n] = cosf(phi);
        lut[32 * WM_MAX_DECIM + n] = -sinf(phi);
    }
    A(hipMemcpyAsync(c->d_lut, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    A(hipStreamSynchronize(c->stream));                      /* k0_taps, shift_tab, afc_init, act_init, init and lut leave with this function */
    if (e != hipSuccess) return fail(c, WMBUS_EDEVICE, "initialisation failed: %s", hipGetErrorString(e));

    c->decs.resize((size_t)c->S * 4);                        /* [stream][chain][algo] */
    for (size_t i = 0; i < c->decs.size(); i++) {
        wm_decoder_init(&c->decs[i].dec, (i >> 1) & 1u ? WM_MODE_S1 : WM_MODE_T1C1);
        c->decs[i].owed = 0; c->decs[i].fed = 0; c->decs[i].lev = wmbus_level{};
    }
    return WMBUS_OK;
}

int wmbus_open(const wmbus_cfg *cfg, wmbus_ctx **out)
{
    if (!cfg || !out) return WMBUS_EINVAL;
    wmbus_ctx *c = new wmbus_ctx();
    c->cfg = *cfg;
    *out = c;                                                /* after a refusal the caller reads the message, then closes */
    std::vector<int16_t> k0_taps;
    int rc = open_validate(c, k0_taps);
    if (!rc) rc = open_geometry(c);
    if (!rc) rc = open_allocate(c);
    if (!rc) rc = open_init(c, k0_taps);
    return rc;
}

void *wmbus_alloc_pinned(size_t nbytes)
{
    void *p = nullptr;
    return hipHostMalloc(&p, nbytes) == hipSuccess ? p : nullptr;
}

void wmbus_free_pinned(void *p) { if (p) hipHostFree(p); }

/* what wmbus_stage and wm_stage_all ask of a copy of `nbytes` per stream, of which the caller holds `room` */
static int stage_check(wmbus_ctx *c, size_t nbytes, size_t room)
{
    if (nbytes > c->cfg.max_push_bytes || nbytes % WMBUS_BLOCK_BYTES || room < nbytes) return fail(c, WMBUS_EINVAL, "stage: nbytes must be a multiple of 4096 and <= max_push_bytes");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    /* with one input window the kernels of a push in flight still read it; with two (cfg.input_windows = 2) the next
     * push is staged into the other one while they run */
    if (c->in_flight && c->n_win == 1) return fail(c, WMBUS_EINVAL, "stage: a push is in flight and the context has one input window (cfg.input_windows = 2 overlaps them)");
    return WMBUS_OK;
}

/* Every stream's bytes of the next push in ONE copy (the batch's host-sourced path: a context's streams lie `pitch` apart in
 * its page-locked slab and in_stride apart in HBM -- a pitched copy; 128 copies of 1-2 MiB per context-push were 1024
 * copy commands per step of the batch CLI).  Same rules as wmbus_stage. */
static int wm_stage_all(wmbus_ctx *c, const uint8_t *slab, size_t pitch, size_t nbytes)
{
    if (!c || !slab) return WMBUS_EINVAL;
    if (const int rc = stage_check(c, nbytes, pitch)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(wmbus_device_input(c, 0), c->k0.on ? c->k0.raw_stride : c->in_stride, slab, pitch, nbytes, c->NC, hipMemcpyHostToDevice, c->copy_stream));
    return WMBUS_OK;
}

void *wmbus_device_input(wmbus_ctx *c, unsigned stream)
{
    if (!c || stream >= c->NC) return nullptr;               /* by capture; a context with channels always has a K0 stage */
    if (c->k0.on) return c->k0.d_raw + ((size_t)c->fill * c->NC + stream) * c->k0.raw_stride;     /* raw bytes: K0 fills the pipeline's window */
    return c->d_in + ((size_t)c->fill * c->S + stream) * c->in_stride + WM_HIST_BYTES;
}

int wmbus_stage(wmbus_ctx *c, unsigned stream, const uint8_t *cu8, size_t nbytes)
{
    if (!c || stream >= c->NC || !cu8) return WMBUS_EINVAL;
    if (const int rc = stage_check(c, nbytes, nbytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(wmbus_device_input(c, stream), cu8, nbytes, hipMemcpyHostToDevice, c->copy_stream));
    return WMBUS_OK;
}

/* ---- launches --------------------------------------------------------------------------------- */
static float *ema_carry(wmbus_ctx *c, bool out) { return c->d_ema_carry + (size_t)(c->carry_in ^ (out ? 1u : 0u)) * 2 * c->S; }
static void *st_carry(wmbus_ctx *c, int algo, bool out)
{
    const Framer &f = c->fr[algo];
    return (char *)f.d_st_carry + (size_t)(c->carry_in ^ (out ? 1u : 0u)) * 2 * c->S * f.state_bytes;
}

/* EMA hand-offs between tiles (k1_verify), the first uncertified tile of every row into the repair list (k1_collect),
 * its length into scalar `cnt`.  A listed tile is re-run sequentially from its predecessor's exact tail, which may
 * uncover the next one: exact by construction. */
static void ema_verify(wmbus_ctx *c, uint32_t cnt)
{
    const uint32_t rows = 2 * c->S, ntiles = c->ntiles;
    wm_launch(c, k1_verify, dim3((rows + 63) / 64, ntiles), dim3(64), 0, c->d_ema_head, c->d_ema_tail, ema_carry(c, false), ntiles, rows, c->d_first_bad);
    wm_launch(c, k1_collect, dim3((rows + 63) / 64), dim3(64), 0, c->d_first_bad, ntiles, rows, c->S, c->d_list_ema, c->d_scalars + cnt);
}

static int ema_repair(wmbus_ctx *c, uint32_t cnt)          /* list launch: a fixed grid walks d_list[0 .. scalar cnt) */
{
    K1Args k1 = c->k1a;
    k1.relist = c->d_list_ema; k1.n_relist = c->d_scalars + cnt;
    return launch_k1(c, K1_REPAIR, k1, dim3(16, 1));
}

static void ema_commit(wmbus_ctx *c)
{
    wm_launch(c, k1_commit, dim3((2 * c->S + 63) / 64), dim3(64), 0, c->d_ema_tail, ema_carry(c, true), c->ntiles, 2 * c->S);
}

/* Does the launch that reads the re-run list whose length is scalar `cnt` walk chains (K2Args.bad), or re-run every listed segment on its own?
 * The framers' FIRST list round is the parallel one -- except the run-length framer's with -s (fr_launch has the measurements). */
static bool list_walks_chains(const wmbus_ctx *c, int algo, uint32_t cnt)
{
    return cnt != c->fr[algo].sc + c->fr[algo].round0 || (algo == WMBUS_ALGO_RLA && c->cfg.simultaneous);
}

static void fr_verify(wmbus_ctx *c, int algo, uint32_t cnt)
{
    const Framer &f = c->fr[algo];
    const K2Args &a = f.k2;
    const uint32_t lanes = 2u * a.g.nseg[algo] * a.g.S;
    wm_launch(c, k2_verify, dim3((lanes + 255) / 256), dim3(256), 0, a.g, (uint32_t)algo, (const uint32_t *)a.st_start,
                       (const uint32_t *)a.st_final, f.state_bytes / 4u, f.d_list, c->d_scalars + cnt, f.d_bad, list_walks_chains(c, algo, cnt) ? 1u : 0u);
}

/* one framer's kernel alone: every lane (cnt == ~0) or the re-run list whose length is scalar `cnt` */
static void fr_launch(wmbus_ctx *c, int algo, uint32_t cnt)
{
    K2Args a = c->fr[algo].k2;
    const uint32_t lanes = 2u * a.g.nseg[algo] * a.g.S;
    const bool all = cnt == 0xFFFFFFFFu;
    a.list = all ? nullptr : c->fr[algo].d_list;
    a.n_lanes = lanes; a.n_ptr = all ? nullptr : c->d_scalars + cnt;
    /* The run-length framer's FIRST list round re-runs every listed segment on its own, in parallel, from its predecessor's
     * end state as recorded: a neighbour that is listed too usually comes out of its re-run with the end state it had (the
     * framer resets inside the segment), so that state was right all along -- walking such runs serially made the round twice
     * as long on the bench workload (r04 A/B: 133 against 147 Gsamples/s).  What is STILL listed after that round is a true
     * cascade (a burst longer than a segment): from the second list round on a listed lane walks its chain (rla_lanes). */
    /* ... except with -s (round 6): S1 telegrams lie in both chains' bands there, a telegram is a run of twenty to forty listed segments, and
     * re-running each of them on its own from a predecessor that is wrong as well is work in vain: 10 994 lanes in the first round, 5 088
     * walking their chains in the second.  With the walk in the FIRST round the second finds 2 lanes (configs[2] at batch size: 174-177 ->
     * 181-182 Gsamples/s, run-length stage 9.9 -> 8.3 ms). */
    if (!all && !list_walks_chains(c, algo, cnt)) a.bad = nullptr;      /* (the clock kernel's first list round is parallel too: clock_lanes) */
    /* (Round 5 tried a middle way for the clock kernel's first round: parallel, but a lane whose end state came out new carries it
     * on into an UNLISTED successor.  The second round shrank from 7 to 4 lanes and the job lost 1.8 %: 170.0 against 173.1.) */
    /* list launches: blocks for 3/16 of the lanes (a re-run list is a few percent of them; the blocks walk whatever is more) */
#ifdef WM_DBG_SKIP_CLOCK                                      /* timing experiment only (tools/build_variant.sh): from the fourth push on no clock-recovery launch at all --
                                                             * what the clock kernels' place on the GPU costs the rest of the job.  The output is wrong. */
    if (algo == WMBUS_ALGO_T2A && c->push_seq > 3) return;
#endif
#ifdef WM_DBG_SKIP_RLA
    if (algo == WMBUS_ALGO_RLA && c->push_seq > 3) return;
#endif
    /* the systolic form of the clock kernel: a block of four waves per 64 lanes (wm_k2_clock_sys.h); the others: a lane per thread */
    const bool sys = algo == WMBUS_ALGO_T2A && c->clk_form == 4u, dc = c->flags & WM_F_DC, coop = a.g.S % 64u == 0u;      /* coop: whole waves of captures load cooperatively */
    void (*k)(K2Args);
    if (algo == WMBUS_ALGO_RLA) k = all ? k2_rla : k2_rla_list;
    else if (!sys) k = all ? (dc ? k2_clock<true> : k2_clock<false>) : (dc ? k2_clock_list<true> : k2_clock_list<false>);
    else if (!all) k = dc ? k2_clock_sys_list<true> : k2_clock_sys_list<false>;
    else k = dc ? (coop ? k2_clock_sys<true, true> : k2_clock_sys<true, false>) : (coop ? k2_clock_sys<false, true> : k2_clock_sys<false, false>);
    const uint32_t B = sys ? 256u : 64u * (algo == WMBUS_ALGO_RLA ? WM_RLA_WPB : WM_CLK_WPB), per = sys ? 64u : B;      /* threads, lanes per block */
    const uint32_t grid = all ? (lanes + per - 1u) / per : std::max(sys ? 64u : 16u, (lanes / per) * 3u / 16u);
    /* the form a batch lane launches for two contexts at once (wm_k_pair.h): the run-length framer's and the systolic clock kernel's */
    void (*kp)(WmPair<K2Args>) = nullptr;
    if (algo == WMBUS_ALGO_RLA) kp = all ? k2_rla_pair : k2_rla_list_pair;
    else if (sys && !all) kp = dc ? k2_clock_sys_list_pair<true> : k2_clock_sys_list_pair<false>;
    else if (sys) kp = dc ? (coop ? k2_clock_sys_pair<true, true> : k2_clock_sys_pair<true, false>) : (coop ? k2_clock_sys_pair<false, true> : k2_clock_sys_pair<false, false>);
    const uint32_t lds = sys ? (uint32_t)sizeof(ClkSysLds) : 0u;
    if (!kp) { wm_launch(c, k, dim3(grid), dim3(B), lds, a); return; }
    wm_launch_pairable(c, [=](hipStream_t st) { hipLaunchKernelGGL(k, dim3(grid), dim3(B), lds, st, a); }, kp, dim3(grid), B, lds, a);
}

static void fr_carry(wmbus_ctx *c)
{
    const uint32_t rows = 2u * c->S;
    for (int al = 1; al >= 0; al--) {
        const Framer &f = c->fr[al];
        const WmPush &g = f.k2.g;
        if (al == WMBUS_ALGO_T2A || (c->flags & WM_F_RLA))
            wm_launch(c, k_carry, dim3((rows + 255) / 256), dim3(256), 0, (const uint32_t *)f.k2.st_final,
                               (uint32_t *)st_carry(c, al, true), f.state_bytes / 4u, rows, g.nseg_cap[al], g.nseg[al]);
        else   /* a disabled run-length framer keeps its state */
        {
            void *const dst = st_carry(c, al, true), *const src = st_carry(c, al, false);
            const size_t n = (size_t)rows * f.state_bytes;
            (void)wm_op(c, "hipMemcpyAsync", [=] { return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream); });
        }
    }
}

/* K3 on the settled chip streams: chips-per-framer sums, access-code hits, bursts (decoded on the GPU where they are
 * complete), then the scalars for the host.  Nothing here needs a number from the host. */
static int launch_k3(wmbus_ctx *c, bool again)
{
    const WmPush &g = c->last;
    if (again) {                                             /* collect's slow path: the counters of the first attempt go */
        wm_memset(c, c->d_scalars + SC_NHITS, 0, 5 * sizeof(uint32_t));          /* NHITS .. NBYTES */
        wm_memset(c, c->d_scalars + SC_CHIPS, 0, 6 * sizeof(uint32_t));          /* CHIPS, RS_N, RS_FAIL */
        /* ... and so does its burst-storage warning (chips dropped by the framers stay dropped: that bit is kept) */
        wm_launch(c, k_and_word, dim3(1), dim3(1), 0, c->d_scalars + SC_ERR, ~(uint32_t)WM_ERR_BURST_OVERFLOW);
    }
    wm_launch(c, k_sum_counts, dim3(std::min(64u, (2u * (c->fr[0].nseg_cap + c->fr[1].nseg_cap) * c->S + 255u) / 256u)), dim3(256), 0, g,
                       c->fr[0].d_counts, c->fr[1].d_counts, c->d_scalars + SC_CHIPS);
    /* grid.y: the parts a region is scanned in -- the run-length framer's regions can be longer than their capacity (spill chunks) */
    const uint32_t scan_parts = (std::max(g.cap[0] + WM_SPILL_LEVELS * WM_SPILL_CHUNK, g.cap[1]) + WM_K3_SCAN_PART - 1u) / WM_K3_SCAN_PART;
    {
        const K3ScanArgs sa{g, c->fr[0].d_chips, c->fr[1].d_chips, c->fr[0].d_counts, c->fr[1].d_counts, c->fr[0].d_sync_seen, c->fr[1].d_sync_seen, c->d_hits,
                            c->d_scalars + SC_NHITS, c->hits_cap, c->d_scalars + SC_ERR};
        const dim3 grid((2u * (g.nseg[0] + g.nseg[1]) * g.S + 255u) / 256u, scan_parts);
        wm_launch_pairable(c, [=](hipStream_t st) {
            hipLaunchKernelGGL(k3_scan, grid, dim3(256), 0, st, sa.g, sa.chips0, sa.chips1, sa.counts0, sa.counts1, sa.seen0, sa.seen1, sa.hits, sa.n_hits, sa.hits_cap, sa.err);
        }, k3_scan_pair, grid, 256u, 0u, sa);
    }
    K3Args k3{};
    k3.g = g; k3.rssi = c->d_rssi;
    for (int al = 0; al < 2; al++) { k3.chips[al] = c->fr[al].d_chips; k3.counts[al] = c->fr[al].d_counts; }
    k3.hits = c->d_hits; k3.n_hits = c->d_scalars + SC_NHITS; k3.hits_cap = c->hits_cap; k3.pending = c->d_pending;
    k3.hdr = (WmBurstHdr *)c->dv_hdr; k3.hdr_cap = c->hdr_cap; k3.words = (uint32_t *)c->dv_words; k3.words_cap = c->words_cap;
    k3.n_hdr = c->d_scalars + SC_NHDR; k3.n_words = c->d_scalars + SC_NWORDS; k3.err = c->d_scalars + SC_ERR;
    if (c->gpu_decode) {
        k3.pkts = (WmPkt *)c->dv_pkts; k3.pkts_cap = c->pkts_cap; k3.bytes = (uint8_t *)c->dv_bytes; k3.bytes_cap = c->bytes_cap;
        k3.n_pkts = c->d_scalars + SC_NPKTS; k3.n_bytes = c->d_scalars + SC_NBYTES;
    }
    if (c->lev_on) { k3.lev_pkt = c->d_lev_src_pkts; k3.lev_hdr = c->d_lev_src_hdr; }
    if (c->rs_this && !c->rs_full_now) {
        k3.plans = c->d_plans;
        /* RSSI on demand: which tiles do the bursts touch (k3_spans), then their RSSI (an RS = 2 launch of the demodulation
         * kernel over the list, a fixed grid), then the bursts */
        wm_memset(c, c->d_rs_flags, 0, (size_t)c->ntiles * c->S * sizeof(uint32_t));
        {
            const K3SpansArgs sp{k3, c->T, c->ntiles, c->d_rs_flags, c->d_rs_list, c->d_scalars + SC_RS_N};
            const dim3 grid(std::max(1u, std::min((4 * c->S + c->hits_cap + 3u) / 4u, (uint32_t)WM_K3_BLOCKS)));
            wm_launch_pairable(c, [=](hipStream_t st) { hipLaunchKernelGGL(k3_spans, grid, dim3(256), 0, st, sp.a, sp.tile_len, sp.ntiles, sp.flags, sp.list, sp.n_list); },
                               k3_spans_pair, grid, 256u, 0u, sp);
        }
        K1Args k1 = c->k1a;
        k1.relist = c->d_rs_list; k1.n_relist = c->d_scalars + SC_RS_N;
        wm_record(c, c->ev[EV_RS]);
        const int rc = launch_k1(c, K1_RSSI, k1, dim3(std::max(1u, std::min((uint32_t)WM_RS_BLOCKS, c->ntiles * c->S)), 1));    /* r04 A/B: 512 / 1024 / 2048 / 4096 blocks: no difference */
        if (rc) return rc;
        wm_record(c, c->ev[EV_RS_END]);
    }
    /* Few blocks: a latency-bound wave parked on a SIMD costs the demodulation kernel one of its eight wave slots there
     * for as long as it lives; 256 blocks put one on every SIMD of the chip (r02 sweep: 256 -> 64 blocks + 6 %, 16 blocks - 9 %: then the kernel itself becomes the longest link of the chain) */
    const uint32_t most = 4 * c->S + c->hits_cap;
    {
        const K3BurstsArgs ba{k3, 0xFFFFFFFFu};
        const dim3 grid(std::max(1u, std::min((most + 3u) / 4u, (uint32_t)WM_K3_BLOCKS)));
        wm_launch_pairable(c, [=](hipStream_t st) { hipLaunchKernelGGL(k3_bursts, grid, dim3(256), 0, st, ba.a, ba.n_items_host); }, k3_bursts_pair, grid, 256u, 0u, ba);
    }
    if (c->lev_on) {
        /* cfg.line_levels: a level per record k3_bursts has written (it left every record's access-code sample in d_lev_src_*), from this push's soft symbols and the tail in front of them; then the
         * tail for the next push (into the other half: collect's slow path comes through here again and must find the same tail) */
        K3LevArgs lv{};
        lv.g = g; lv.dphi = c->d_dphi;
        lv.tail_in = c->d_lev_tail + (size_t)c->carry_in * 2 * c->S * WM_LEV_TAIL; lv.tail_out = c->d_lev_tail + (size_t)(c->carry_in ^ 1u) * 2 * c->S * WM_LEV_TAIL;
        lv.src_pkts = k3.pkts ? k3.lev_pkt : nullptr; lv.n_pkts = k3.n_pkts; lv.pkts_cap = k3.pkts_cap;
        lv.src_hdr = k3.lev_hdr; lv.n_hdr = k3.n_hdr; lv.hdr_cap = k3.hdr_cap;
        lv.lev_pkts = (WmLevel *)c->dv_lev_pkts; lv.lev_hdr = (WmLevel *)c->dv_lev_hdr;
        wm_launch(c, k3_levels, dim3(std::max(1u, std::min((most + 3u) / 4u, (uint32_t)WM_K3_BLOCKS))), dim3(256), 0, lv);
        wm_launch(c, k3_level_tail, dim3((WM_LEV_TAIL + 255u) / 256u, 2u * c->S), dim3(256), 0, lv);
        if (c->rep_on && k3.pkts) {
            /* cfg.crc_repair: behind the bursts and the levels, on the packets k3_bursts has just written (in place: their flags, their
             * bytes), with the same soft symbols and the same tail as the levels; a record per packet slot beside them */
            K3RepArgs ra{};
            ra.k3 = k3; ra.dphi = lv.dphi; ra.tail_in = lv.tail_in; ra.src_pkts = k3.lev_pkt; ra.rep_pkts = (WmRepair *)c->dv_rep_pkts;
            wm_launch(c, k3_repair, dim3(std::max(1u, std::min((most + 3u) / 4u, (uint32_t)WM_K3_BLOCKS))), dim3(256), 0, ra);
        }
        if (c->res_on && k3.pkts) {
            /* cfg.s1_rescue: on the abort records k3_bursts has just written (in place: flags, off, sample, rssi_now; status and consumed
             * stay), its bytes appended to the arena -- before the counters go to the host.  k3_repair and k3_quality take a rescued
             * record for the abort it still is, so the order among the three does not matter */
            K3ResArgs ra{};
            ra.k3 = k3; ra.dphi = lv.dphi; ra.src_pkts = k3.lev_pkt; ra.res_pkts = (WmRescue *)c->dv_res_pkts;
            wm_launch(c, k3_rescue, dim3(std::max(1u, std::min((most + 3u) / 4u, (uint32_t)WM_K3_BLOCKS))), dim3(256), 0, ra);
        }
        if (c->q_on && k3.pkts) {
            /* cfg.line_quality: a record per packet slot from the chip regions, the counts and the soft symbols -- nothing k3_repair
             * changes, so its place behind it is a matter of order only */
            K3QualArgs qa{};
            qa.k3 = k3; qa.dphi = lv.dphi; qa.src_pkts = k3.lev_pkt; qa.q_pkts = (WmQuality *)c->dv_q_pkts;
            wm_launch(c, k3_quality, dim3(std::max(1u, std::min((most + 3u) / 4u, (uint32_t)WM_K3_BLOCKS))), dim3(256), 0, qa);
        }
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

/* A context with a K0 stage: the launch arguments of K0 for a push of `raw_bytes`, and the host's copy of the counters moved on.  Returns the
 * bytes the pipeline gets from this push: the whole 4096-byte blocks of (remainder + what this push produces); may be 0. */
static size_t k0_plan(wmbus_ctx *c, size_t raw_bytes, K0Args *ka)
{
    auto &k = c->k0;
    const uint32_t n_in = (uint32_t)(raw_bytes / k.bps);
    const uint64_t out_end = ((k.n_in + n_in) * (uint64_t)k.L + k.M - 1u) / k.M;      /* output n exists once input floor(n M / L) is in: n M < pushed L */
    const uint32_t n_out = (uint32_t)(out_end - k.n_out);
    const size_t total = (size_t)k.rem + 2u * (size_t)n_out, whole = total / WMBUS_BLOCK_BYTES * WMBUS_BLOCK_BYTES;
    *ka = K0Args{};
    ka->raw = k.d_raw + (size_t)c->fill * c->NC * k.raw_stride; ka->raw_stride = k.raw_stride;
    ka->out = c->d_in + (size_t)c->fill * c->S * c->in_stride + WM_HIST_BYTES; ka->out_stride = c->in_stride;
    ka->taps = k.d_taps;
    if (k.resample) { ka->hist_in = k.d_hist + (size_t)k.cur * c->S * (k.T - 1u); ka->hist_out = k.d_hist + (size_t)(k.cur ^ 1u) * c->S * (k.T - 1u); }
    ka->rem_in = k.d_rem + (size_t)k.cur * c->S * WMBUS_BLOCK_BYTES; ka->rem_out = k.d_rem + (size_t)(k.cur ^ 1u) * c->S * WMBUS_BLOCK_BYTES;
    ka->n_first = k.n_out; ka->in_first = k.n_in; ka->n_in = n_in; ka->n_out = n_out;
    ka->rem_prev = k.rem; ka->keep_from = (uint32_t)whole;
    ka->L = k.L; ka->M = k.M; ka->T = k.T; ka->tile = k.tile;
    ka->gain_q8 = k.gain; ka->clipped = c->d_scalars + SC_CLIP;
    ka->step = k.step; ka->shift_tab = k.d_shift_tab;
    if (k.chan) { ka->n_ch = c->CH; for (uint32_t ch = 0; ch < c->CH; ch++) ka->steps[ch] = k.steps[ch]; }
    if (k.dc) {                                          /* a push is whole 4096-byte blocks: whole level blocks */
        ka->dc_tab = k.d_dc_tab; ka->dc_stride = k.dc_stride;
        k.dca = K0DcArgs{ka->raw, k.raw_stride, k.d_dc_sums, k.d_dc_tab, k.d_dc_state + (size_t)k.cur * c->NC, k.d_dc_state + (size_t)(k.cur ^ 1u) * c->NC,
                         k.dc_stride, n_in >> WM_K0_DC_LOG2, k.dc};
    }
    if (k.agc) {
        ka->agc_tab = k.d_agc_tab; ka->dc_stride = k.dc_stride;
        k.aga = K0AgcArgs{ka->raw, k.raw_stride, k.d_dc_tab, k.d_agc_tab, k.dc_stride, n_in >> WM_K0_DC_LOG2};
    }
    if (c->afc.on) {                                     /* the dc / agc tables are runtime branches of the AFC form: dc_stride is set above where either is on */
        ka->afc = c->afc.d_push;
        c->afc.args = K0AfcArgs{c->spec.d_peak, c->spec.d_blocks, c->afc.d_state + (size_t)k.cur * c->afc.n, c->afc.d_state + (size_t)(k.cur ^ 1u) * c->afc.n,
                                c->afc.d_push, c->afc.fin, c->afc.nominal, c->afc.range, n_in, nullptr, nullptr, 0u, {}, {}};
        if (c->afc.chan) {
            c->afc.args.n_ch = c->CH;
            for (uint32_t ch = 0; ch < c->CH; ch++) { c->afc.args.ch_nominal_hz[ch] = c->cfg.input_channel_hz[ch]; c->afc.args.ch_range_hz[ch] = c->afc.ch_range[ch]; }
        }
        if (c->spec.age) { c->afc.args.peak1 = c->spec.d_peak + 2u * c->spec.slot_stride; c->afc.args.blocks1 = c->spec.d_blocks + c->spec.slot_stride; }
    }
    k.last_out = 2ull * n_out * c->S;
    k.n_in += n_in; k.n_out = out_end; k.rem = (uint32_t)(total - whole); k.cur ^= 1u;
    k.last_bytes = whole; k.last_win = c->fill;
    return whole;
}

/* cfg.input_spectrum: the survey over the `n_blk` level blocks every capture has in this push, raw bytes at raw + capture x raw_stride.  With
 * a blocker it runs behind k0_dc_plan (it subtracts that table).  A wave takes a run of consecutive level blocks and ends with 512 64-bit
 * atomic adds and 512 atomic maxima, which at runs of 4 cost as much as the transform (1.40 against 0.78 ms; 64 is no
 * better than 16): runs of 16 where that still leaves a wave for every SIMD of the chip (16384 level blocks in the push), else of 4 (a live
 * stream's single capture: 1024 level blocks per push are 256 waves then, not 64 -- there the launch is latency, not throughput). */
#ifndef WM_K0_SPEC_RUN
#define WM_K0_SPEC_RUN 16          /* build-time A/B (tools/build_variant.sh) */
#endif
static int spec_launch(wmbus_ctx *c, const uint8_t *raw, uint64_t raw_stride, uint32_t n_blk)
{
#define K0_SPEC_AGE(DC) {k0_spectrum<WM_K0_CU8, DC, true>, k0_spectrum<WM_K0_CS8, DC, true>, k0_spectrum<WM_K0_CS16, DC, true>, k0_spectrum<WM_K0_CF32, DC, true>}
    void (*const aged[2][4])(K0SpecArgs) = {K0_SPEC_AGE(false), K0_SPEC_AGE(true)};       /* cfg.input_spectrum_age */
#undef K0_SPEC_AGE
    void (*const kernel[2][4])(K0SpecArgs) = {{k0_spectrum<WM_K0_CU8, false>, k0_spectrum<WM_K0_CS8, false>, k0_spectrum<WM_K0_CS16, false>, k0_spectrum<WM_K0_CF32, false>},
                                              {k0_spectrum<WM_K0_CU8, true>, k0_spectrum<WM_K0_CS8, true>, k0_spectrum<WM_K0_CS16, true>, k0_spectrum<WM_K0_CF32, true>}};
    /* cfg.line_power: the band form of either */
#define K0_SPEC_BANDS(DC, AGE) {k0_spectrum<WM_K0_CU8, DC, AGE, true>, k0_spectrum<WM_K0_CS8, DC, AGE, true>, k0_spectrum<WM_K0_CS16, DC, AGE, true>, k0_spectrum<WM_K0_CF32, DC, AGE, true>}
    void (*const banded[2][2][4])(K0SpecArgs) = {{K0_SPEC_BANDS(false, false), K0_SPEC_BANDS(true, false)}, {K0_SPEC_BANDS(false, true), K0_SPEC_BANDS(true, true)}};      /* [age][dc][fmt] */
#undef K0_SPEC_BANDS
    K0SpecArgs a{};
    a.raw = raw; a.raw_stride = raw_stride;
    a.dc_tab = c->k0.dc ? c->k0.d_dc_tab : nullptr; a.dc_stride = c->k0.dc_stride;
    a.shift_tab = c->k0.d_shift_tab;
    a.sum = c->spec.d_sum; a.peak = c->spec.d_peak; a.blocks = c->spec.d_blocks;
    a.n_blk = n_blk; a.run = (uint64_t)n_blk * c->NC >= 16384u ? (uint32_t)WM_K0_SPEC_RUN : 4u;
    if (!n_blk) return WMBUS_OK;
    if (c->spec.age) {
        /* the one place where a push's level blocks enter the ageing survey, once per push: what the push clears and what it leaves out
         * is k0_spec_age_plan's decision, and K moves on here and nowhere else */
        const K0SpecAgePlan plan = k0_spec_age_plan(c->spec.K, n_blk, c->spec.age);
        a.age = c->spec.age; a.k_first = c->spec.K; a.e_keep = plan.e_keep; a.slot_stride = c->spec.slot_stride;
        c->spec.K += n_blk;
        if (plan.clear == 3u) wm_memset(c, c->spec.d_slots, 0, (size_t)2 * c->spec.slot_stride * sizeof(uint64_t));
        else if (plan.clear) wm_memset(c, c->spec.d_slots + (plan.clear >> 1) * c->spec.slot_stride, 0, (size_t)c->spec.slot_stride * sizeof(uint64_t));
    }
    if (c->pw.on) {
        /* the one place where a push's level blocks enter the waterfall: K moves on here and nowhere else */
        if (n_blk > c->pw.blk_cap) return fail(c, WMBUS_EINVAL, "internal error: a push of %u level blocks, the band rows hold %u", n_blk, c->pw.blk_cap);
        a.bands = c->pw.d_bands; a.band_stride = (uint64_t)WM_K0_POW_BANDS * c->pw.blk_cap;
        c->pw.last_first = c->pw.K; c->pw.last_blk = n_blk; c->pw.K += n_blk;
    }
    const uint32_t runs = (n_blk + a.run - 1u) / a.run;
    wm_launch(c, c->pw.on ? banded[c->spec.age != 0u][c->k0.dc != 0u][c->k0.fmt] : (c->spec.age ? aged : kernel)[c->k0.dc != 0u][c->k0.fmt], dim3((runs + WM_K0_SPEC_WAVES - 1u) / WM_K0_SPEC_WAVES, c->NC), dim3(64u * WM_K0_SPEC_WAVES), 0, a);
    return WMBUS_OK;
}

/* cfg.line_power: P of this push's level blocks for every pipeline row, behind the survey's band rows and -- where there is one -- behind
 * k0_afc_plan, whose committed state names the centre this push is rotated to; then P to pinned host memory, on the context's stream. */
static int power_launch(wmbus_ctx *c)
{
    auto &w = c->pw;
    const uint32_t n_blk = w.last_blk;
    if (!n_blk) return WMBUS_OK;
    K0PowArgs a{};
    a.bands = w.d_bands; a.band_stride = (uint64_t)WM_K0_POW_BANDS * w.blk_cap;
    a.P = w.d_P; a.p_stride = w.blk_cap;
    a.afc = c->afc.on ? c->afc.args.st_out : nullptr;
    a.S = c->S; a.n_ch = c->CH; a.n_blk = n_blk; a.in_hz = w.fin;
    if (c->k0.chan) for (uint32_t ch = 0; ch < c->CH; ch++) a.centre_hz[ch] = c->cfg.input_channel_hz[ch];
    else a.centre_hz[0] = c->cfg.input_shift_hz;
    if (c->cfg.simultaneous) { a.chain_hz[WMBUS_CHAIN_T1C1] = WM_K0_POW_SIM_HZ; a.chain_hz[WMBUS_CHAIN_S1] = -WM_K0_POW_SIM_HZ; }
    w.args = a;
    wm_launch(c, k0_channel_power, dim3((n_blk + WM_K0_POW_THREADS / 32u - 1u) / (WM_K0_POW_THREADS / 32u), c->S, 2u), dim3(WM_K0_POW_THREADS), 0, a);
    HIPCHK(c, hipGetLastError());
    {
        uint32_t *const h_P = w.h_P, *const d_P = w.d_P;
        const size_t pitch = (size_t)w.blk_cap * sizeof(uint32_t), width = (size_t)n_blk * sizeof(uint32_t), rows = (size_t)2 * c->S;
        WM_OP(c, "hipMemcpy2DAsync", [=] { return hipMemcpy2DAsync(h_P, pitch, d_P, pitch, width, rows, hipMemcpyDeviceToHost, c->stream); });
    }
    if (c->act.on) {
        /* cfg.channel_activity: the rows' state moves on over this push's P, here and nowhere else -- once per push, as pw.K does */
        K0ActArgs ca{};
        ca.P = w.d_P; ca.p_stride = w.blk_cap; ca.n_blk = n_blk; ca.rows = 2u * c->S;
        ca.T = c->act.T; ca.H = c->act.H;
        ca.st = c->act.d_state; ca.arena = c->act.d_arena; ca.count = c->act.d_count; ca.base = c->act.taken; ca.cap = c->act.cap;
        wm_launch(c, k0_activity, dim3(2u * c->S), dim3(64u), 0, ca);
        HIPCHK(c, hipGetLastError());
        wm_memcpy(c, c->act.h_count, c->act.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost);
        c->act.launched = true;
    }
    return WMBUS_OK;
}

static int k0_launch(wmbus_ctx *c, const K0Args &ka)
{
    /* [cfg.input_dc != 0][cfg.input_shift_hz != 0][WMBUS_FMT_*]; cfg.input_agc: the same three in the tables below */
#define K0_FORMATS(K, ...) {K<WM_K0_CU8, __VA_ARGS__>, K<WM_K0_CS8, __VA_ARGS__>, K<WM_K0_CS16, __VA_ARGS__>, K<WM_K0_CF32, __VA_ARGS__>}
    void (*const resample_agc[2][2][4])(K0Args) = {{K0_FORMATS(k0_resample_agc, false, false), K0_FORMATS(k0_resample_agc, true, false)},
                                                   {K0_FORMATS(k0_resample_agc, false, true), K0_FORMATS(k0_resample_agc, true, true)}};
    void (*const convert_agc[2][2][4])(K0Args) = {{K0_FORMATS(k0_convert_agc, false, false), K0_FORMATS(k0_convert_agc, true, false)},
                                                  {K0_FORMATS(k0_convert_agc, false, true), K0_FORMATS(k0_convert_agc, true, true)}};
    void (*const gain[2][4])(K0AgcArgs) = {K0_FORMATS(k0_agc_gain, false), K0_FORMATS(k0_agc_gain, true)};
#undef K0_FORMATS
    void (*const resample[2][2][4])(K0Args) = {
        {{k0_resample, k0_resample_fmt<WM_K0_CS8>, k0_resample_fmt<WM_K0_CS16>, k0_resample_fmt<WM_K0_CF32>},
         {k0_resample_shift<WM_K0_CU8>, k0_resample_shift<WM_K0_CS8>, k0_resample_shift<WM_K0_CS16>, k0_resample_shift<WM_K0_CF32>}},
        {{k0_resample_dc<WM_K0_CU8, false>, k0_resample_dc<WM_K0_CS8, false>, k0_resample_dc<WM_K0_CS16, false>, k0_resample_dc<WM_K0_CF32, false>},
         {k0_resample_dc<WM_K0_CU8, true>, k0_resample_dc<WM_K0_CS8, true>, k0_resample_dc<WM_K0_CS16, true>, k0_resample_dc<WM_K0_CF32, true>}}};
    void (*const convert[2][2][4])(K0Args) = {
        {{k0_convert<WM_K0_CU8>, k0_convert<WM_K0_CS8>, k0_convert<WM_K0_CS16>, k0_convert<WM_K0_CF32>},
         {k0_convert_shift<WM_K0_CU8>, k0_convert_shift<WM_K0_CS8>, k0_convert_shift<WM_K0_CS16>, k0_convert_shift<WM_K0_CF32>}},
        {{k0_convert_dc<WM_K0_CU8, false>, k0_convert_dc<WM_K0_CS8, false>, k0_convert_dc<WM_K0_CS16, false>, k0_convert_dc<WM_K0_CF32, false>},
         {k0_convert_dc<WM_K0_CU8, true>, k0_convert_dc<WM_K0_CS8, true>, k0_convert_dc<WM_K0_CS16, true>, k0_convert_dc<WM_K0_CF32, true>}}};
    /* cfg.input_channels: [WMBUS_FMT_*] -- the blocker and the AGC are runtime branches of these (K0Args.dc_tab / agc_tab); the grid's y is
     * the pipeline stream, the level kernels' the capture */
    void (*const resample_ch[4])(K0Args) = {k0_resample_ch<WM_K0_CU8>, k0_resample_ch<WM_K0_CS8>, k0_resample_ch<WM_K0_CS16>, k0_resample_ch<WM_K0_CF32>};
    void (*const convert_ch[4])(K0Args) = {k0_convert_ch<WM_K0_CU8>, k0_convert_ch<WM_K0_CS8>, k0_convert_ch<WM_K0_CS16>, k0_convert_ch<WM_K0_CF32>};
    /* cfg.input_afc: [WMBUS_FMT_*] -- the blocker and the AGC are runtime branches of these too */
    void (*const resample_afc[4])(K0Args) = {k0_resample_afc<WM_K0_CU8>, k0_resample_afc<WM_K0_CS8>, k0_resample_afc<WM_K0_CS16>, k0_resample_afc<WM_K0_CF32>};
    void (*const convert_afc[4])(K0Args) = {k0_convert_afc<WM_K0_CU8>, k0_convert_afc<WM_K0_CS8>, k0_convert_afc<WM_K0_CS16>, k0_convert_afc<WM_K0_CF32>};
    /* cfg.input_channel_afc_hz: [WMBUS_FMT_*] -- the channels form with k0_afc_plan's {step, base} per pipeline stream */
    void (*const resample_ch_afc[4])(K0Args) = {k0_resample_ch_afc<WM_K0_CU8>, k0_resample_ch_afc<WM_K0_CS8>, k0_resample_ch_afc<WM_K0_CS16>, k0_resample_ch_afc<WM_K0_CF32>};
    void (*const convert_ch_afc[4])(K0Args) = {k0_convert_ch_afc<WM_K0_CU8>, k0_convert_ch_afc<WM_K0_CS8>, k0_convert_ch_afc<WM_K0_CS16>, k0_convert_ch_afc<WM_K0_CF32>};
    if (c->k0.dc) {                                      /* the level blocks' sums, then the recurrence over them: the table the K0 kernel subtracts */
        void (*const sums[4])(K0DcArgs) = {k0_dc_sums<WM_K0_CU8>, k0_dc_sums<WM_K0_CS8>, k0_dc_sums<WM_K0_CS16>, k0_dc_sums<WM_K0_CF32>};
        const K0DcArgs &da = c->k0.dca;
        wm_launch(c, sums[c->k0.fmt], dim3((da.n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), c->NC), dim3(WM_K0_THREADS), 0, da);
        wm_launch(c, k0_dc_plan, dim3(c->NC), dim3(128), 0, da);
        c->k0.last_dc_blocks = da.n_blk;
    }
    if (c->spec.on) { const int rc = spec_launch(c, ka.raw, ka.raw_stride, ka.n_in >> WM_K0_DC_LOG2); if (rc) return rc; }      /* per capture, in front of the rotation, behind the blocker's table */
    /* cfg.input_afc: every capture's {step, base} for this push from its max-hold as it stands now, and the state commit, in ONE short launch */
    if (c->afc.on) wm_launch(c, k0_afc_plan, dim3(c->NC, c->afc.chan ? c->CH : 1u), dim3(WM_K0_AFC_THREADS), 0, c->afc.args);
    if (c->pw.on) { const int rc = power_launch(c); if (rc) return rc; }
    if (c->k0.agc) {                                     /* every level block's gain from its peak, behind the blocker: the table the K0 kernel's output stage reads */
        const K0AgcArgs &ga = c->k0.aga;
        wm_launch(c, gain[c->k0.dc != 0u][c->k0.fmt], dim3((ga.n_blk + WM_K0_THREADS / 64u - 1u) / (WM_K0_THREADS / 64u), c->NC), dim3(WM_K0_THREADS), 0, ga);
        c->k0.last_dc_blocks = ga.n_blk;
    }
    const auto &stage = c->k0.agc ? (c->k0.resample ? resample_agc : convert_agc) : (c->k0.resample ? resample : convert);
    void (*const kernel)(K0Args) = c->afc.chan ? (c->k0.resample ? resample_ch_afc : convert_ch_afc)[c->k0.fmt]
                                   : c->afc.on  ? (c->k0.resample ? resample_afc : convert_afc)[c->k0.fmt]
                                   : c->k0.chan ? (c->k0.resample ? resample_ch : convert_ch)[c->k0.fmt]
                                              : stage[c->k0.dc != 0u][c->k0.shift][c->k0.fmt];
    wm_launch(c, kernel, dim3((ka.n_out + ka.tile - 1u) / ka.tile, c->S), dim3(WM_K0_THREADS), c->k0.resample ? c->k0.lds : 0u, ka);
    HIPCHK(c, hipGetLastError());
    c->k0.launches++;
    return WMBUS_OK;
}

static int enqueue_front_impl(wmbus_ctx *c, size_t nbytes)
{
    if (nbytes == 0 || nbytes > c->cfg.max_push_bytes || nbytes % WMBUS_BLOCK_BYTES)
        return fail(c, WMBUS_EINVAL, "process: nbytes must be a positive multiple of 4096 and <= max_push_bytes");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "process: previous push not collected");
    HIPCHK(c, hipSetDevice(c->cfg.device));            /* HIP's current device is per host thread; a context may be driven from any */
    if (c->poisoned) return fail(c, WMBUS_EDEVICE, "process: an earlier internal error left this context unusable; close it");
    K0Args k0a{};
    if (c->k0.on) nbytes = k0_plan(c, nbytes, &k0a);   /* from here on nbytes counts RESAMPLED bytes: what the pipeline sees (0: no whole block yet) */
    gettimeofday(&c->arrival, nullptr);
    if (c->committed) { c->carry_in ^= 1u; c->committed = false; }     /* the previous push's end state is this one's start state */
    const uint32_t n_new = (uint32_t)(nbytes / 2);
    uint8_t *win = c->d_in + (size_t)c->fill * c->S * c->in_stride;      /* the window wmbus_stage has been filling */
    WmPush g{};
    g.in = win; g.in_stride = c->in_stride; g.n0 = c->n0; g.m0 = c->n0 / c->d;
    g.n_new = n_new; g.M = (uint32_t)((c->n0 + n_new) / c->d - g.m0);
    g.Mcap = c->Mcap; g.d = c->d; g.S = c->S; g.lut_n = 32 * c->d;
    g.lut_phase0 = (uint32_t)((13ull * (c->n0 % g.lut_n)) % g.lut_n);
    g.flags = c->flags;
    for (int al = 0; al < 2; al++) {
        const Framer &f = c->fr[al];
        g.seg_len[al] = f.C; g.nseg[al] = (g.M + f.C - 1) / f.C; g.nseg_cap[al] = f.nseg_cap; g.cap[al] = f.cap;
    }
    g.warm[0] = c->cfg.warmup_t1c1; g.warm[1] = c->cfg.warmup_s1; g.lookback = c->cfg.rla_lookback;
    g.s1_span = 1u;                                     /* (2: S1 clock lanes over two segments -- built and measured in rounds 2-4, -2 %: the kernels keep the form) */
    g.sp.arena = c->d_spill; g.sp.arena_words = c->spill_words; g.sp.chain = c->d_chain; g.sp.nchain = c->d_nchain;
    g.sp.used = c->d_nchain + (size_t)2 * c->S * c->fr[0].nseg_cap;
    c->last = g; c->have_last = true;
    c->n_hdr = c->n_words = c->n_pkts = 0;
    c->enqueued = true;                                 /* from here on a failure leaves half a push on the stream: the context is poisoned */

    /* the staged bytes arrive on the copy stream */
    if (c->copy_stream != c->stream) {
        WM_OP(c, "hipEventRecord(ev_staged, copy_stream)", [=] { return hipEventRecord(c->ev_staged, c->copy_stream); });
        wm_wait(c, c->ev_staged);
    }
    wm_record(c, c->ev[EV_PUSH]);
    wm_launch(c, k_copy_hist, dim3(c->S), dim3(256), 0, c->d_hist, (uint64_t)WM_HIST_BYTES, (uint64_t)0, win, c->in_stride);
    if (c->k0.on && g.M == 0) {                          /* a push that completes no block: K0 alone, and its clip count */
        wm_memset(c, c->d_scalars + SC_CLIP, 0, sizeof(uint32_t));
        const int rc0 = k0_launch(c, k0a);
        if (rc0) return rc0;
        wm_memcpy(c, c->h_scalars + SC_CLIP, c->d_scalars + SC_CLIP, sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    if (g.M > 0) {
        wm_memset(c, c->d_scalars, 0, c->zero_words * sizeof(uint32_t));     /* scalars, region flags, spill chains */
        /* K1 */
        const uint32_t T = c->T, ntiles = (g.M + T - 1) / T;
        c->ntiles = ntiles;
        /* on demand pays while the bursts touch a minority of the tiles (an RS = 2 tile costs a third of a full one, and the
         * first pass saves a seventh): a context that has just listed more than cfg.rssi_dense_pm per mille of them (configs[2]: S1
         * telegrams of 30-100 ms in both chains) takes the full pass for the next sixteen pushes, then looks again
         * (r04 visit: configs[2] lists 31 % of its tiles and loses 7 % on demand -- its front end, five input samples per decimated one
         * through the -s rotation, is most of the kernel; the bench workload lists 11 % and gains 5-7 %) */
        c->rs_this = c->rs_od && c->rs_pause == 0;
        if (c->rs_pause) c->rs_pause--;
        c->k1a = K1Args{g, c->d_dphi, c->d_rssi, c->d_lut, c->d_lut + 32 * WM_MAX_DECIM, c->d_ema_head, c->d_ema_tail, ntiles, c->d_scalars + SC_ERR,
                        nullptr, ema_carry(c, false), nullptr, 0u, c->d_rs_flags, ema_carry(c, true), c->d_scalars + SC_RS_FAIL};
        int rc;
        {
            K1Turn turn(c, k1_chain[c->cfg.device]);
            if ((rc = turn.take())) return rc;
            wm_record(c, c->ev[EV_K1]);
            if (c->k0.on) { rc = k0_launch(c, k0a); if (rc) return rc; }      /* inside demod_ms: the demodulation kernel reads what it writes */
            /* the survey of a context on the plain cu8 path reads the device input window itself (a push of that path is whole 4096-byte
             * blocks and always has decimated samples: this branch is taken); the context stays on the plain path */
            else if (c->spec.on) {
                rc = spec_launch(c, win + WM_HIST_BYTES, c->in_stride, (uint32_t)(nbytes / 2u) >> WM_K0_DC_LOG2); if (rc) return rc;
                if (c->pw.on) { rc = power_launch(c); if (rc) return rc; }
            }
            /* The hand-over of the turn costs 0.15-0.2 ms (the next context's stream sits in an event wait on another
             * hardware queue; r03 trace: median 128 us between one K1 and the next, eight times per step = 5 % of it).
             * So the turn is handed over EARLY: a push's tiles leave in two launches, the event the next context waits for
             * lies behind the first, and the last k1_tail_pm per mille of the tiles run while the hand-over is under
             * way -- beside the head of the next context's K1 at most.
             * r04 A/B: exact 152.5 / 153.2 against 149.1 / 150.1 Gsamples/s with 60 per mille (30: 151.6 / 152.0, 120: 151.0 / 152.3, 250:
             * 148.9 / 147.4); tolerance mode, whose K1 is a third of the length, 170.1 / 171.9 against 171.0 / 173.0: off there */
            const bool big = c->rs_this && c->k1_big;            /* the first pass without the RSSI on 2000-sample tiles (wm_k1_demod.h K1GeoT) */
            const uint32_t T1 = big ? (uint32_t)WM_K1_TILE_BIG : T, nt1 = (g.M + T1 - 1) / T1;
            const uint32_t n_tail = std::min(nt1 - 1u, (uint32_t)((uint64_t)nt1 * c->k1_tail_pm / 1000u));
            K1Args k1 = c->k1a;
            const K1Role role = c->rs_this ? K1_FIRST : K1_FULL;
            /* the first pass without the RSSI takes several consecutive tiles per block: the input of a block's next tile is on
             * its way while the current one is computed (wm_k1_demod.h, K1Args.tpb) */
            const uint32_t tpb = c->rs_this && c->d >= 2 && c->d <= 5 ? c->k1_tpb : 1u;
            k1.tpb = tpb; k1.tile_end = nt1 - n_tail;
#ifdef WM_DBG_SKIP_K1                                       /* timing experiment only (tools/build_variant.sh): from the fourth push on the framers run on the
                                                             * soft symbols the third push left -- what a context's chain costs without any demodulation kernel
                                                             * beside it.  The output is wrong. */
            const bool dbg_skip = c->push_seq > 3;
#else
            const bool dbg_skip = false;
#endif
            rc = dbg_skip ? 0 : launch_k1(c, role, k1, dim3((nt1 - n_tail + tpb - 1u) / tpb, c->S));
            if (rc) return rc;
            if (n_tail && !dbg_skip) {
                wm_record(c, c->ev_turn);
                k1.tile0 = nt1 - n_tail; k1.tile_end = nt1;
                rc = launch_k1(c, role, k1, dim3((n_tail + tpb - 1u) / tpb, c->S));
                if (rc) return rc;
            }
            wm_record(c, c->ev[EV_K1_END]);
            if ((rc = turn.hand_on(n_tail ? c->ev_turn : c->ev[EV_K1_END]))) return rc;
        }
        /* Everything behind K1 is enqueued while it runs -- no step of a push waits for the host any more:
         * hand-off verification makes its first rounds on the device (counters per round), K3 reads its item
         * count there, the results land in pinned host memory.  wmbus_collect looks at the last counters. */
        c->rs_full_now = false;
        if (!c->rs_this) {                                      /* (on demand: the RSSI comes behind the framers, launch_k3) */
            for (unsigned r = 0; r < c->ema_rounds && c->opt_rounds; r++) {
                ema_verify(c, SC_EMA + r);
                rc = ema_repair(c, SC_EMA + r);
                if (rc) return rc;
            }
            ema_verify(c, SC_EMA + c->ema_rounds);
            ema_commit(c);
        }

        /* K2: clock recovery + time2 framer (also produces the slicer bits the RLA needs) */
        K2Args k2{};                                        /* what both framers share; the rest is Framer's */
        k2.g = g; k2.dphi = c->d_dphi; k2.rssi = c->d_rssi; k2.bits = c->d_bits;
        k2.err = c->d_scalars + SC_ERR;
        k2.ckpt = c->d_ckpt; k2.nck = c->nck;
        for (int al = 0; al < 2; al++) {
            Framer &f = c->fr[al];
            f.k2 = k2;
            f.k2.algo = (uint32_t)al; f.k2.bad = f.d_bad;
            f.k2.chips = f.d_chips; f.k2.counts = f.d_counts; f.k2.sync_seen = f.d_sync_seen;
            f.k2.st_start = f.d_st_start; f.k2.st_final = f.d_st_final; f.k2.st_carry = st_carry(c, al, false);
        }
        /* One stream, one launch after the other: clock first pass, its unattended re-run rounds, then the run-length framer and its
         * rounds.  (Rounds 2-4 built and measured the alternatives -- the clock re-run lanes and the run-length framer fused into one
         * launch; the run-length framer on a side stream beside the clock rounds -- both shorten a context's chain of launches by
         * 4-5 ms and both LOSE: the job is bound by the ring of demodulation kernels, and more streams or fatter launches only
         * get in its way; DESIGN_HISTORY.md.  Round 5 brought the fused launch back once more, with the demodulation kernel 13 % shorter and
         * a context's chain the bound: 155-161 against 172 Gsamples/s, the demodulation kernel in region 3.8-4.0 instead of 3.3 ms.) */
        const bool rla = c->flags & WM_F_RLA;
        for (int al = 1; al >= (rla ? 0 : 1); al--) {
            const Framer &f = c->fr[al];
            wm_record(c, c->ev[al ? EV_CLK : EV_RLA]);
            fr_launch(c, al, 0xFFFFFFFFu);                           /* the first pass */
            /* (a push of one segment per row has no hand-off inside it: its only lane starts from the carried state -- no rounds to enqueue;
             * a live stream's 2^16-sample pushes are such) */
            for (unsigned r = f.round0; r < f.rounds && c->opt_rounds && g.nseg[al] > 1u; r++) { fr_verify(c, al, f.sc + r); fr_launch(c, al, f.sc + r); }
        }
        if (rla) {
            /* the last verification of either framer and both carries in one launch (k2_finish) */
            K2Finish fin{};
            for (int al = 0; al < 2; al++) {
                const Framer &f = c->fr[al];
                fin.st_start[al] = (const uint32_t *)f.k2.st_start; fin.st_final[al] = (const uint32_t *)f.k2.st_final;
                fin.words[al] = f.state_bytes / 4u;
                fin.carry[al] = (uint32_t *)st_carry(c, al, true); fin.verify[al] = 1u; fin.do_carry[al] = 1u;
                fin.list[al] = f.d_list; fin.n_list[al] = c->d_scalars + f.sc + f.rounds; fin.bad[al] = f.d_bad;
                fin.heads[al] = list_walks_chains(c, al, f.sc + f.rounds);
            }
            const uint32_t most = std::max(2u * g.S, 2u * std::max(g.nseg[0], g.nseg[1]) * g.S);
            wm_launch(c, k2_finish, dim3((most + 255u) / 256u), dim3(256), 0, g, fin);
            wm_record(c, c->ev[EV_FR_END]);
        } else {
            wm_record(c, c->ev[EV_RLA]);
            wm_memset(c, c->fr[0].d_counts, 0, (size_t)2 * c->S * c->fr[0].nseg_cap * sizeof(uint32_t));
            fr_verify(c, WMBUS_ALGO_T2A, c->fr[1].sc + c->fr[1].rounds);
            wm_record(c, c->ev[EV_FR_END]);
            fr_carry(c);
        }
        c->committed = true;
    }
    /* the next push sees the last 4096 staged bytes in front of it */
    wm_launch(c, k_copy_hist, dim3(c->S), dim3(256), 0, win, c->in_stride, (uint64_t)nbytes, c->d_hist, (uint64_t)WM_HIST_BYTES);
    HIPCHK(c, hipGetLastError());
    c->fill = (c->fill + 1) % c->n_win;
    c->n0 += n_new;
    c->push_seq++;
    c->in_flight = true; c->back_due = true;
    return WMBUS_OK;
}

/* BACK of a push: what needs the host decoders' state after the previous push -- the chips half-received telegrams are
 * still owed -- then K3 on the settled chip streams and the scalars for the host. */
static int enqueue_back_impl(wmbus_ctx *c)
{
    if (!c->back_due) return WMBUS_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->back_due = false;
    if (c->last.M > 0) {
        for (uint32_t s = 0; s < c->S; s++)
            for (int ch = 0; ch < 2; ch++)
                for (int al = 0; al < 2; al++)
                    c->h_pending[(al * 2 + ch) * c->S + s] = c->decs[((size_t)s * 2 + ch) * 2 + al].owed;
        wm_memcpy(c, c->d_pending, c->h_pending, 4 * c->S * sizeof(uint32_t), hipMemcpyHostToDevice);
        wm_record(c, c->ev[EV_K3]);
        const int rc = launch_k3(c, false);
        if (rc) return rc;
        wm_record(c, c->ev[EV_K3_END]);
        wm_memcpy(c, c->h_scalars, c->d_scalars, SC_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost);
        wm_record(c, c->ev[EV_D2H_END]);
    }
    return WMBUS_OK;
}

/* a failure after the first enqueue leaves half a push on the stream and the carried state undefined */
static int enqueue_front(wmbus_ctx *c, size_t nbytes)
{
    c->enqueued = false;
    const int rc = enqueue_front_impl(c, nbytes);
    if (rc && c->enqueued) c->poisoned = true;
    return rc;
}
static int enqueue_back(wmbus_ctx *c)
{
    const int rc = enqueue_back_impl(c);
    if (rc) c->poisoned = true;
    return rc;
}

int wmbus_process(wmbus_ctx *c, size_t nbytes)
{
    if (!c) return WMBUS_EINVAL;
    const int rc = enqueue_front(c, nbytes);
    return rc ? rc : enqueue_back(c);
}

/* The optimistic rounds of wmbus_process left work: finish it round by round with the host in the loop (rare: a
 * cascade of hand-off failures longer than the rounds enqueued), then redo what depended on it. */
static int finish_slowly(wmbus_ctx *c, bool ema_left, bool left[2], bool rs_left = false)      /* left: [WMBUS_ALGO_*] */
{
    auto read_scalars = [&]() -> int {
        HIPCHK(c, hipMemcpyAsync(c->h_scalars, c->d_scalars, SC_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    /* verify once more, counting in SC_SLOW (cleared behind whatever launch has just read it); algo < 0: the RSSI filter's hand-offs */
    auto recheck = [&](int algo, uint32_t *n) -> int {
        wm_launch(c, k_copy_word, dim3(1), dim3(1), 0, c->d_scalars + SC_SLOW, 0u);
        if (algo < 0) ema_verify(c, SC_SLOW); else fr_verify(c, algo, SC_SLOW);
        const int rc = read_scalars();
        *n = c->h_scalars[SC_SLOW];
        return rc;
    };
    const uint32_t max_rounds = std::max({c->ntiles, c->last.nseg[0], c->last.nseg[1]}) + 4;
    /* re-run the list whose length is scalar `cnt` (the list of the last verify of its kind is still there), verify, and again until nothing is listed */
    auto settle = [&](int algo, uint32_t cnt, unsigned *tally, const char *what) -> int {
        for (uint32_t round = 0, n = 0;; round++, cnt = SC_SLOW) {
            *tally += c->h_scalars[cnt];
            int rc = 0;
            if (algo < 0) rc = ema_repair(c, cnt); else fr_launch(c, algo, cnt);
            if (rc || (rc = recheck(algo, &n))) return rc;
            if (n == 0) return 0;
            if (round > max_rounds) return fail(c, WMBUS_EDEVICE, "%s did not converge", what);
        }
    };
    int rc;
    if (rs_left) {
        /* RSSI on demand, and a lane whose value is read could not prove it (wm_k1_demod.h: constant input can keep the bracket
         * open): this push's RSSI the long way -- the full kernel over every tile, its hand-offs verified against the carried
         * state and repaired like any other context's */
        uint32_t n = 0;
        if ((rc = launch_k1(c, K1_FULL, c->k1a, dim3(c->ntiles, c->S))) || (rc = recheck(-1, &n))) return rc;
        ema_left = n != 0;
        if (!ema_left) ema_commit(c);
        c->rs_full_now = true;
    }
    if (ema_left) {
        if ((rc = settle(-1, rs_left ? (uint32_t)SC_SLOW : SC_EMA + c->ema_rounds, &c->tim.ema_retries, "RSSI filter hand-off repair"))) return rc;
        ema_commit(c);
    }
    for (int algo = 1; algo >= 0; algo--) {                    /* clock first: with -o the slicer words depend on it */
        const Framer &f = c->fr[algo];
        if (left[algo] && (rc = settle(algo, f.sc + f.rounds, algo ? &c->tim.clock_reruns : &c->tim.rla_reruns, "segment verification"))) return rc;
        if (left[algo] && algo == WMBUS_ALGO_T2A && (c->flags & WM_F_DC) && (c->flags & WM_F_RLA)) {
            /* the run-length framer ran on slicer words that the clock re-runs have just replaced: all of it again */
            const uint32_t last = c->fr[0].sc + c->fr[0].rounds;
            fr_launch(c, WMBUS_ALGO_RLA, 0xFFFFFFFFu);
            wm_launch(c, k_copy_word, dim3(1), dim3(1), 0, c->d_scalars + last, 0u);
            fr_verify(c, WMBUS_ALGO_RLA, last);
            if ((rc = read_scalars())) return rc;
            left[0] = c->h_scalars[last] != 0;
        }
    }
    fr_carry(c);
    if ((rc = launch_k3(c, true)) || (rc = read_scalars())) return rc;
    /* the chips have changed, so have the bursts and the tiles they touch: one of those may be unprovable in turn */
    bool none[2] = {false, false};
    if (c->rs_this && !c->rs_full_now && c->h_scalars[SC_RS_FAIL]) return finish_slowly(c, false, none, true);
    return 0;
}

/* cfg.channel_activity: the records the push has closed, from the arena's ticket order into rows ascending, first_block ascending.  Only a
 * push that closed any pays the second copy. */
static int activity_collect(wmbus_ctx *c)
{
    auto &t = c->act;
    t.bursts.clear();
    if (!t.launched) return WMBUS_OK;
    t.launched = false;
    const uint32_t n = *t.h_count - t.taken;
    t.taken = *t.h_count;
    if (n > t.cap) { c->poisoned = true; return fail(c, WMBUS_EDEVICE, "internal error: %u activity records, the arena holds %u", n, t.cap); }
    if (!n) return WMBUS_OK;
    t.raw.resize(n);
    HIPCHK(c, hipMemcpyAsync(t.raw.data(), t.d_arena, (size_t)n * sizeof(K0ActRecord), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::sort(t.raw.begin(), t.raw.end(), [](const K0ActRecord &x, const K0ActRecord &y) { return x.row != y.row ? x.row < y.row : x.first_block < y.first_block; });
    for (const K0ActRecord &r : t.raw) {
        const uint32_t v = r.row % c->S;
        wmbus_burst b{};
        b.first_block = r.first_block; b.blocks = r.blocks; b.mean = r.mean; b.floor = r.floor;
        b.stream = v / c->CH; b.channel = (uint8_t)(v % c->CH); b.chain = (uint8_t)(r.row / c->S);
        t.bursts.push_back(b);
    }
    return WMBUS_OK;
}

/* First half of wmbus_collect: wait for the push, finish leftover hand-off rounds, read the counters.  Afterwards the
 * candidate telegrams sit in pinned host memory and nothing of this push is left on the GPU. */
static int wait_gpu(wmbus_ctx *c)
{
    c->done.valid = false;
    if (!c->in_flight) return WMBUS_OK;
    if (c->back_due) { const int rc = enqueue_back(c); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->in_flight = false;
    c->tim = wmbus_timing{};
    if (c->act.on) { const int rc = activity_collect(c); if (rc) return rc; }
    if (c->pw.on && c->pw.last_blk) {                        /* this push's P behind the history: the last pw.hist level blocks in front of it stay */
        auto &w = c->pw;
        const size_t drop = w.ring[0].size() > w.hist ? w.ring[0].size() - w.hist : 0u;      /* ring_first + size == last_first: every push's level blocks pass through here once */
        for (size_t r = 0; r < w.ring.size(); r++) {
            std::vector<uint32_t> &v = w.ring[r];
            v.erase(v.begin(), v.begin() + drop);
            v.insert(v.end(), w.h_P + r * w.blk_cap, w.h_P + r * w.blk_cap + w.last_blk);
        }
        w.ring_first += drop;
        w.got_first = w.last_first; w.got_blk = w.last_blk; w.last_blk = 0;
    }
    if (c->k0.on) { c->tim.input_bytes_out = c->k0.last_out; c->tim.input_clipped = c->h_scalars[SC_CLIP]; }
    if (c->last.M > 0) {
        auto span = [&](int from, int to) { float ms = 0; hipEventElapsedTime(&ms, c->ev[from], c->ev[to]); return ms; };
        c->tim.demod_ms = span(EV_K1, EV_K1_END);
        c->tim.turn_wait_ms = span(EV_PUSH, EV_K1);          /* on the GPU: behind the other contexts' demodulation kernels */
        c->tim.clock_ms = span(EV_CLK, EV_RLA);              /* the clock kernel's launches */
        c->tim.rla_ms = span(EV_RLA, EV_FR_END);             /* the run-length framer's */
        if (c->rs_this) c->tim.rssi_ms = span(EV_RS, EV_RS_END);
        c->tim.gather_ms = span(EV_K3, EV_K3_END);
        c->tim.d2h_ms = span(EV_K3_END, EV_D2H_END);
        c->tim.gpu_total_ms = span(EV_PUSH, EV_D2H_END);
        const uint32_t *hs = c->h_scalars;
#ifdef WM_DBG_WALK_STATS
        if (c->push_seq == 4) {
            unsigned h[2][32];
            hipMemcpyFromSymbol(h, HIP_SYMBOL(wm_walk_hist), sizeof h);
            for (int ch = 0; ch < 2; ch++) {
                fprintf(stderr, "run-length walks so far, %s chain, by segments walked:", ch ? "S1" : "T1/C1");
                for (int i = 1; i < 32; i++) fprintf(stderr, " %u", h[ch][i]);
                fprintf(stderr, "\n");
            }
        }
#endif
        for (unsigned r = 0; r < c->ema_rounds; r++) c->tim.ema_retries += hs[SC_EMA + r];
        unsigned *const reruns[2] = {&c->tim.rla_reruns, &c->tim.clock_reruns}, *const per_round[2] = {c->tim.rla_round, c->tim.clock_round};
        bool left[2];
        for (int al = 0; al < 2; al++) {
            const Framer &f = c->fr[al];
            for (unsigned r = f.round0; r < f.rounds; r++) *reruns[al] += hs[f.sc + r];
            for (unsigned r = 0; r < 4; r++) per_round[al][r] = f.round0 + r < f.rounds ? hs[f.sc + f.round0 + r] : 0u;
            left[al] = hs[f.sc + f.rounds] != 0;
        }
        const bool ema_left = hs[SC_EMA + c->ema_rounds];
        const bool rs_left = c->rs_this && hs[SC_RS_FAIL] != 0;
        c->tim.rssi_mode = c->rs_this ? WMBUS_RSSI_ON_DEMAND : c->rs_od ? WMBUS_RSSI_PAUSED : WMBUS_RSSI_EVERY_SAMPLE;
        if (c->rs_this) {
            c->tim.rssi_tiles = hs[SC_RS_N];
            const uint32_t dense_pm = c->cfg.rssi_dense_pm ? c->cfg.rssi_dense_pm : 200u;
            if ((uint64_t)hs[SC_RS_N] * 1000u > (uint64_t)dense_pm * c->ntiles * c->S) c->rs_pause = 16;
        }
        if (ema_left || left[0] || left[1] || rs_left) {
            const int rc = finish_slowly(c, ema_left, left, rs_left);
            if (rc) { c->poisoned = true; return rc; }
            c->tim.slow_path = 1;
            if (c->rs_full_now) c->tim.rssi_mode = WMBUS_RSSI_FELL_BACK;
        }
        const uint32_t err = hs[SC_ERR];
        if (err & WM_ERR_CHIP_OVERFLOW) {            /* a time2 region over its proven bound: a defect, not an input property */
            c->poisoned = true;
            return fail(c, WMBUS_EDEVICE, "internal error: time2 chip region overflow (err=%u)", err);
        }
        /* storage exhausted (spill arena / burst arena): chips or candidate bursts were dropped; every carried state
         * is exact, so the stream goes on -- reported, never fatal (the reference never gives up either) */
        c->tim.warnings = ((err & WM_ERR_CHIP_TRUNC) ? WMBUS_WARN_CHIPS_DROPPED : 0u) | ((err & WM_ERR_BURST_OVERFLOW) ? WMBUS_WARN_BURSTS_DROPPED : 0u);
        c->n_hdr = std::min(hs[SC_NHDR], c->hdr_cap); c->n_words = hs[SC_NWORDS]; c->n_pkts = std::min(hs[SC_NPKTS], c->pkts_cap);
        for (int al = 0; al < 2; al++) for (int ch = 0; ch < 2; ch++) c->tim.chips[ch][al] = hs[SC_CHIPS + al * 2 + ch];
    }
    c->tim.bursts = c->n_hdr + c->n_pkts;
    c->done.n_hdr = c->n_hdr; c->done.n_pkts = c->n_pkts; c->done.m_end = c->last.m0 + c->last.M; c->done.arrival = c->arrival; c->done.seq = c->push_seq;
    c->done.valid = true;
    return WMBUS_OK;
}

int wmbus_collect(wmbus_ctx *c)
{
    if (!c) return WMBUS_EINVAL;
    const int rc = wait_gpu(c);
    if (rc) { c->lines.clear(); c->text.clear(); c->levels.clear(); c->powers.clear(); c->repairs.clear(); c->rescues.clear(); c->res_subjects = c->res_rescued = 0; c->qualities.clear(); return rc; }
    return decode_host(c);
}

/* The host half of wmbus_collect -- sort, strip / format, merge -- over the records of the context's LAST push again, `reps` times, with no
 * GPU work at all: how many lines per second the host side sustains when several ranks' contexts decode at once (eight
 * GPUs' worth of lines through one host; tools/host_replay.py).  The persistent packet decoders are put back after every repetition; the
 * lines of the last one stay readable through wmbus_lines.  Returns the number of lines of one repetition, or a negative code. */
long wmbus_debug_replay_decode(wmbus_ctx *c, unsigned reps, double *seconds)
{
    if (!c) return WMBUS_EINVAL;
    const std::vector<HostDecoder> saved = c->decs;
    const double t0 = now_ms();
    long n = 0;
    for (unsigned r = 0; r < reps; r++) {
        c->decs = saved;
        c->done.valid = true;
        const int rc = decode_host(c);
        if (rc) return rc;
        n = (long)c->lines.size();
    }
    if (seconds) *seconds = (now_ms() - t0) * 1e-3;
    return n;
}

size_t wmbus_lines(const wmbus_ctx *c, const wmbus_line **lines)
{
    if (!c) return 0;
    if (lines) *lines = c->lines.data();
    return c->lines.size();
}

size_t wmbus_line_levels(const wmbus_ctx *c, const wmbus_level **levels)
{
    if (levels) *levels = c && c->lev_on ? c->levels.data() : nullptr;
    return c && c->lev_on ? c->levels.size() : 0;
}

size_t wmbus_line_repairs(const wmbus_ctx *c, const wmbus_repair **records)
{
    if (records) *records = c && c->rep_on ? c->repairs.data() : nullptr;
    return c && c->rep_on ? c->repairs.size() : 0;
}

size_t wmbus_line_rescues(const wmbus_ctx *c, const wmbus_rescue **records)
{
    if (records) *records = c && c->res_on ? c->rescues.data() : nullptr;
    return c && c->res_on ? c->rescues.size() : 0;
}

int wmbus_rescue_stats(const wmbus_ctx *c, unsigned *subjects, unsigned *rescued)
{
    if (subjects) *subjects = 0;
    if (rescued) *rescued = 0;
    if (!c || !c->res_on) return WMBUS_EINVAL;
    if (subjects) *subjects = c->res_subjects;
    if (rescued) *rescued = c->res_rescued;
    return WMBUS_OK;
}

size_t wmbus_line_quality(const wmbus_ctx *c, const wmbus_quality **records)
{
    if (records) *records = c && c->q_on ? c->qualities.data() : nullptr;
    return c && c->q_on ? c->qualities.size() : 0;
}

size_t wmbus_line_power(const wmbus_ctx *c, const wmbus_power **power)
{
    if (power) *power = c && c->pw.on ? c->powers.data() : nullptr;
    return c && c->pw.on ? c->powers.size() : 0;
}

size_t wmbus_activity(const wmbus_ctx *c, const wmbus_burst **records)
{
    const bool on = c && c->act.on && !c->act.bursts.empty();
    if (records) *records = on ? c->act.bursts.data() : nullptr;
    return on ? c->act.bursts.size() : 0;
}

uint64_t wmbus_activity_progress(const wmbus_ctx *c)
{
    return c && c->act.on ? c->pw.got_first + c->pw.got_blk : 0u;
}

long wmbus_activity_rule(const uint32_t *p, size_t n, unsigned in_hz, unsigned ratio_q8, wmbus_burst *out, size_t cap)
{
    if ((!p && n) || (!out && cap) || in_hz < 800000u || (ratio_q8 && (ratio_q8 < 257u || ratio_q8 > 65535u))) return WMBUS_EINVAL;
    std::vector<K0ActBurst> found;
    k0_activity_rule(p, n, in_hz, ratio_q8 ? ratio_q8 : WM_K0_ACT_RATIO_Q8, found);
    for (size_t i = 0; i < found.size() && i < cap; i++) {
        wmbus_burst b{};
        b.first_block = found[i].first_block; b.blocks = found[i].blocks; b.mean = found[i].mean; b.floor = found[i].floor;
        out[i] = b;
    }
    return (long)found.size();
}

long wmbus_activity_match(const wmbus_burst *records, size_t n, unsigned stream, unsigned channel, int chain, uint64_t ka)
{
    if (!records && n) return WMBUS_EINVAL;
    for (size_t i = 0; i < n; i++)
        if (records[i].stream == stream && records[i].channel == channel && records[i].chain == chain && k0_activity_matches(records[i].first_block, records[i].blocks, ka))
            return (long)i;
    return -1;
}

long wmbus_read_waterfall(wmbus_ctx *c, unsigned capture, uint32_t *rows, uint64_t *first_block, size_t cap_rows)
{
    if (!c || capture >= c->NC || !rows) return WMBUS_EINVAL;
    if (!c->pw.on) return fail(c, WMBUS_EINVAL, "read_waterfall: the context was opened without cfg.line_power");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_waterfall: collect the push first");
    const size_t n = std::min(cap_rows, (size_t)c->pw.got_blk);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n) HIPCHK(c, hipMemcpy(rows, c->pw.d_bands + (size_t)capture * WM_K0_POW_BANDS * c->pw.blk_cap, n * WM_K0_POW_BANDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (first_block) *first_block = c->pw.got_first;
    return (long)n;
}

long wmbus_read_channel_power(wmbus_ctx *c, int chain, unsigned stream_v, uint32_t *p, uint64_t *first_block, size_t cap)
{
    if (!c || chain < 0 || chain > 1 || stream_v >= c->S || !p) return WMBUS_EINVAL;
    if (!c->pw.on) return fail(c, WMBUS_EINVAL, "read_channel_power: the context was opened without cfg.line_power");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_channel_power: collect the push first");
    const std::vector<uint32_t> &v = c->pw.ring[(size_t)chain * c->S + stream_v];
    const size_t n = std::min(cap, (size_t)c->pw.got_blk);
    if (n) memcpy(p, v.data() + (v.size() - c->pw.got_blk), n * sizeof(uint32_t));
    if (first_block) *first_block = c->pw.got_first;
    return (long)n;
}

int wmbus_line_power_rule(const uint32_t *p, uint64_t first_block, size_t n, uint64_t ka, uint64_t ke, unsigned in_hz, wmbus_power *out)
{
    if (!out || (!p && n) || in_hz < 800000u) return WMBUS_EINVAL;
    std::vector<uint32_t> scratch;
    power_record(out, k0_line_power_rule(p, first_block, n, ka, ke, in_hz, scratch));
    return WMBUS_OK;
}

int wmbus_line_power_block(unsigned decimation, unsigned input_rate_hz, uint64_t sample, uint64_t *block)
{
    if (!block || decimation < 1 || decimation > WM_MAX_DECIM) return WMBUS_EINVAL;
    unsigned L = 1, M = 1, T = 0;
    if (input_rate_hz && input_rate_hz != decimation * 800000u && k0_design(input_rate_hz, decimation * 800000u, &L, &M, &T, nullptr, 0)) return WMBUS_EINVAL;
    *block = k0_pow_block_of(sample, decimation, L, M);
    return WMBUS_OK;
}

const char *wmbus_lines_text(const wmbus_ctx *c, size_t *len)
{
    if (!c) return "";
    if (len) *len = c->text.size();
    return c->text.c_str();
}

int wmbus_get_timing(const wmbus_ctx *c, wmbus_timing *t)
{
    if (!c || !t) return WMBUS_EINVAL;
    *t = c->tim;
    return WMBUS_OK;
}

long wmbus_read_tap(wmbus_ctx *c, const char *what, int chain, unsigned stream, void *dst, size_t max_elems)
{
    if (!c || !what || !dst || chain < 0 || chain > 1 || stream >= c->S || !c->have_last) return WMBUS_EINVAL;
    if (!c->cfg.keep_taps) return fail(c, WMBUS_EINVAL, "read_tap: the context was opened without cfg.keep_taps");
    hipStreamSynchronize(c->stream);
    const size_t n = std::min<size_t>(max_elems, c->last.M);
    const size_t row = (size_t)chain * c->S + stream;
    if (!strcmp(what, "dphi")) {
        if (hipMemcpy(dst, c->d_dphi + row * c->Mcap, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return WMBUS_EDEVICE;
    } else if (!strcmp(what, "rssi")) {
        if (hipMemcpy(dst, c->d_rssi + row * c->Mcap, n, hipMemcpyDeviceToHost) != hipSuccess) return WMBUS_EDEVICE;
    } else if (!strcmp(what, "bits")) {
        std::vector<uint32_t> w((n + 31) / 32);
        if (hipMemcpy(w.data(), c->d_bits + row * (c->Mcap / 32), w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return WMBUS_EDEVICE;
        for (size_t k = 0; k < n; k++) ((uint8_t *)dst)[k] = (w[k >> 5] >> (k & 31)) & 1u;
    } else return WMBUS_EINVAL;
    return (long)n;
}

long wmbus_read_resampled(wmbus_ctx *c, unsigned stream, uint8_t *out, size_t cap)
{
    if (!c || !out || stream >= c->S) return WMBUS_EINVAL;
    if (!c->cfg.keep_taps || !c->k0.on) return fail(c, WMBUS_EINVAL, "read_resampled: needs cfg.keep_taps and a context that resamples, converts, shifts, removes the input's DC or levels it (cfg.input_rate_hz, input_shift_hz, input_dc, input_agc, input_format, input_gain_q8)");
    if (c->in_flight) return fail(c, WMBUS_EINVAL, "read_resampled: collect the push first");
    const size_t n = std::min(cap, c->k0.last_bytes);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n) HIPCHK(c, hipMemcpy(out, c->d_in + ((size_t)c->k0.last_win * c->S + stream) * c->in_stride + WM_HIST_BYTES, n, hipMemcpyDeviceToHost));
    return (long)n;
}

long wmbus_read_chips(wmbus_ctx *c, int chain, int algo, unsigned stream, uint32_t *dst, uint64_t *pos, size_t max_elems)
{
    if (!c || chain < 0 || chain > 1 || algo < 0 || algo > 1 || stream >= c->S || !c->have_last || !dst) return WMBUS_EINVAL;
    hipStreamSynchronize(c->stream);
    uint32_t *d_dst = nullptr, *d_n = nullptr; uint64_t *d_pos = nullptr;
    if (hipMalloc((void **)&d_dst, max_elems * 4) != hipSuccess || hipMalloc((void **)&d_pos, max_elems * 8) != hipSuccess ||
        hipMalloc((void **)&d_n, 4) != hipSuccess) {
        hipFree(d_dst); hipFree(d_pos); hipFree(d_n);            /* hipFree(nullptr) is a no-op */
        return WMBUS_ENOMEM;
    }
    /* a context without debug views computes the RSSI only in the tiles a packet decoder reads (RSSI on demand): elsewhere its rows hold
     * nothing, so this view shows 0 there instead of what an earlier push left */
    hipLaunchKernelGGL(k4_flatten, dim3(1), dim3(1), 0, c->stream, c->last, (uint32_t)algo, c->fr[algo].d_chips, c->fr[algo].d_counts,
                       /* no RSSI row where the last push computed it on demand only (a paused or fallen-back push ran the full pass: the row is valid) */
                       c->rs_this && !c->rs_full_now ? (const uint8_t *)nullptr : c->d_rssi, c->fr[algo].cap, (uint32_t)chain, stream, d_dst, d_pos, (uint32_t)max_elems, d_n);
    uint32_t n = 0;
    hipStreamSynchronize(c->stream);
    hipMemcpy(&n, d_n, 4, hipMemcpyDeviceToHost);
    const size_t m = std::min<size_t>(n, max_elems);
    hipMemcpy(dst, d_dst, m * 4, hipMemcpyDeviceToHost);
    if (pos) hipMemcpy(pos, d_pos, m * 8, hipMemcpyDeviceToHost);
    hipFree(d_dst); hipFree(d_pos); hipFree(d_n);
    return (long)n;
}

/* Runs the device versions of the exact scalar helpers (wm_exact.h) over n operand pairs so a
 * test can compare them with the host's IEEE / libm results bit for bit. */
int wmbus_selftest_math(int device, const float *a, const float *b, float *o_sqrt, float *o_div, float *o_atan2,
                        float *o_disc, size_t n)
{
    if (wmbus_device_count() <= device || hipSetDevice(device) != hipSuccess) return WMBUS_ENODEVICE;
    float *d[6] = {};
    for (auto &p : d) if (hipMalloc((void **)&p, n * sizeof(float)) != hipSuccess) return WMBUS_ENOMEM;
    hipMemcpy(d[0], a, n * sizeof(float), hipMemcpyHostToDevice);
    hipMemcpy(d[1], b, n * sizeof(float), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d[0], d[1], d[2], d[3], d[4], d[5], (uint32_t)n);
    float *outs[4] = {o_sqrt, o_div, o_atan2, o_disc};
    int rc = hipDeviceSynchronize() == hipSuccess ? WMBUS_OK : WMBUS_EDEVICE;
    for (int k = 0; k < 4; k++) if (hipMemcpy(outs[k], d[2 + k], n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = WMBUS_EDEVICE;
    for (auto &p : d) hipFree(p);
    return rc;
}

int wmbus_selftest_fir(int device, const float *x, float *out, size_t n)
{
    if (wmbus_device_count() <= device || hipSetDevice(device) != hipSuccess) return WMBUS_ENODEVICE;
    if (!x || !out || n == 0 || n > (size_t)K1Geo::T || (n & 3)) return WMBUS_EINVAL;
    float *d_x = nullptr, *d_o = nullptr;
    if (hipMalloc((void **)&d_x, (n + 48) * sizeof(float)) != hipSuccess || hipMalloc((void **)&d_o, 2 * n * sizeof(float)) != hipSuccess) {
        hipFree(d_x); hipFree(d_o);
        return WMBUS_ENOMEM;
    }
    int rc = hipMemcpy(d_x, x, (n + 48) * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? WMBUS_OK : WMBUS_EDEVICE;
    if (rc == WMBUS_OK) {
        hipLaunchKernelGGL(k_selftest_fir, dim3(1), dim3(256), 0, 0, d_x, d_o, (uint32_t)n);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d_o, 2 * n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = WMBUS_EDEVICE;
    }
    hipFree(d_x); hipFree(d_o);
    return rc;
}

long long wmbus_selftest_udiv(int device, uint32_t *first16, unsigned long long *cases)
{
    if (wmbus_device_count() <= device || hipSetDevice(device) != hipSuccess) return WMBUS_ENODEVICE;
    uint32_t *d_res = nullptr, h[36] = {};
    if (hipMalloc((void **)&d_res, sizeof h) != hipSuccess) return WMBUS_ENOMEM;
    long long rc = hipMemset(d_res, 0, sizeof h) == hipSuccess ? WMBUS_OK : WMBUS_EDEVICE;
    if (rc == WMBUS_OK) {
        hipLaunchKernelGGL(k_selftest_udiv, dim3(4092, 16), dim3(256), 0, 0, d_res, 0u);
        hipLaunchKernelGGL(k_selftest_udiv, dim3(8192, 1), dim3(256), 0, 0, d_res, 1u);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d_res, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) rc = WMBUS_EDEVICE;
    }
    hipFree(d_res);
    if (rc != WMBUS_OK) return rc;
    if (first16) std::memcpy(first16, h + 4, 32 * sizeof(uint32_t));
    if (cases) *cases = ((unsigned long long)h[3] << 32) | h[2];
    return (long long)h[0];
}

#ifdef WM_K1_STAMPS
/* -DWM_K1_STAMPS builds only (tools/gpu_k1_stamps.py): the stage intervals the demodulation kernel's waves have left
 * (wm_k1_demod.h), summed over the slots into out8[0 .. 6], optionally cleared. */
int wmbus_debug_k1_stamps(unsigned long long *out8, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return WMBUS_EDEVICE;
    const size_t n = (size_t)WM_K1_STAMP_SLOTS * 8u;
    if (out8) {
        std::vector<unsigned int> h(n);
        if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(wm_k1_stamp_buf), n * sizeof(unsigned int)) != hipSuccess) return WMBUS_EDEVICE;
        for (int k = 0; k < 8; k++) out8[k] = 0;
        for (size_t i = 0; i < n; i++) out8[i & 7u] += h[i];
    }
    if (reset) {
        void *p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(wm_k1_stamp_buf)) != hipSuccess || hipMemset(p, 0, n * sizeof(unsigned int)) != hipSuccess) return WMBUS_EDEVICE;
    }
    return WMBUS_OK;
}
#endif

}  // extern "C"

#include "wm_batch.h"
