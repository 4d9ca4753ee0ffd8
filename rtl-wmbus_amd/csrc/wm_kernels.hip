/*
 * wm_kernels.hip -- gfx950 kernels for the rtl-wmbus hot path.
 *
 *   k0_resample  option (cfg.input_rate_hz): exact integer polyphase resampler, cu8 at any rate -> cu8 at decimation x 800 kHz
 *                in the input window; everything below runs unchanged behind it.    (no counterpart: rtl_wmbus.c:1274-1292)
 *   k0_resample_fmt<cs8 | cs16 | cf32>  the same for cfg.input_format, with cfg.input_gain_q8 in the output stage;
 *   k0_convert<fmt>  the format / gain conversion alone for an input that is at decimation x 800 kHz already; both count the
 *                bytes their clamp changed (wmbus_timing.input_clipped).
 *   k0_resample_shift<fmt> / k0_convert_shift<fmt>  the same two with cfg.input_shift_hz: every input sample rotated once, where it is
 *                staged, by an exact integer rule (a capture tuned off the channel; no counterpart in the reference).
 *   k0_dc_sums<fmt> -> k0_dc_plan -> k0_resample_dc<fmt, shift> / k0_convert_dc<fmt, shift>  cfg.input_dc: the I/Q DC offset of a zero-IF
 *                receiver, estimated per level block of 512 input samples and subtracted where a sample is staged (no counterpart).
 *   k0_agc_gain<fmt, dc> -> k0_resample_agc<fmt, shift, dc> / k0_convert_agc<fmt, shift, dc>  cfg.input_agc: the gain of every level block
 *                of 512 input samples from the block's own peak, in the place of cfg.input_gain_q8 in the output stage (no counterpart).
 *   k0_resample_ch<fmt> / k0_convert_ch<fmt>  cfg.input_channels: the same two stages with one raw capture feeding C pipeline streams, each
 *                rotated by its own phase step (several channels of one wideband capture; the blocker and the AGC, per capture, as runtime
 *                branches; no counterpart).
 *   k0_spectrum<fmt, dc>  cfg.input_spectrum: the channel survey -- an exact integer 512-point windowed DFT of every level block of the raw
 *                input, summed and max-held per capture and bin over the pushes of a context; reads only (no counterpart).
 *   k0_afc_plan -> k0_resample_afc<fmt> / k0_convert_afc<fmt>  cfg.input_afc: behind k0_spectrum, one block per capture turns the
 *                capture's max-hold into its phase step for this very push (the survey's channel rule, a range, a hysteresis); the two
 *                stages rotate with that {step, base} and a push-local sample index (no counterpart).
 *   k1_demod2    time-parallel front end, one 976-sample tile per block: cu8 -> [+-325 kHz
 *                shift] -> integer boxcars -> decimate -> polar discriminator (exact fdlibm
 *                atan2f) -> FIR low-pass -> soft symbol; |s| -> EMA -> RSSI byte.
 *                                  (rtl_wmbus.c:1310-1352, 517-586, 369-392, 475-495, 1066-1067)
 *   k1_demod_ppf the same behind the polyphase pre-filter of ppf.h (option; rtl_wmbus.c:258-294).
 *   k1_verify / k1_collect / k1_commit   certify the EMA hand-offs between tiles; an uncertified
 *                tile is repaired by a list launch of k1 (one lane per chain, sequential).
 *   k2_clock     lane = (chain, stream, time segment): DC remover, slicer, squared-signal IIR
 *                band-pass, clock lock, time2 framer.            (rtl_wmbus.c:497-515, 1059,
 *                336-365, 1089-1111, 806-852)
 *   k2_rla       lane = (chain, stream, time segment): run-length framer with deglitch and
 *                bit-length tracking.                            (rtl_wmbus.c:617-803)
 *   k2_verify    compares each segment's start state with its predecessor's end state; a
 *                segment whose speculative start was wrong is re-run from the true state (and
 *                stops at the first checkpoint of the speculative pass it reproduces).
 *   k3_bursts    access-code hits -> the chips (with their RSSI bytes) a host packet decoder
 *                consumes.   k4_flatten: debug/parity view of a whole chip stream.
 *   k3_levels    option (cfg.line_levels): frequency offset and deviation of every candidate telegram from the soft symbols of its
 *                preamble, in integers; k3_level_tail carries the last 782 soft symbols of every row to the next push.
 *                                  (no counterpart: the reference prints two RSSI bytes only)
 *   k3_repair    option (cfg.crc_repair): a time2 telegram decoded inside the push that fails a block CRC gets its least reliable chips
 *                flipped, 255 patterns per bad block over the lanes of a wave, in integers; the packet is rewritten in place.
 *                                  (no counterpart: the reference prints such a telegram with CRC flag 0)
 *   k3_rescue    option (cfg.s1_rescue): an S1 telegram of the time2 framer aborted at an invalid Manchester pair is decoded again, every
 *                invalid pair decided by the larger of its two soft symbols, one wave per packet; the abort record is rewritten in place.
 *                                  (no counterpart: the reference drops such a telegram)
 *   k3_quality   option (cfg.line_quality): chip rate, jitter of the decision instants and eye of the soft symbols of every time2
 *                telegram decoded inside the push, one wave per packet, two walks over its chips, 64-bit integer sums.
 *                                  (no counterpart: the reference prints two RSSI bytes only)
 *
 * Exactness: every float operation the reference performs is performed here in the same order
 * with separate roundings (wm_exact.h; the file is also built with -ffp-contract=off).  The
 * recurrences (EMA, DC, IIR, run-length state) are evaluated sequentially inside a lane; time
 * parallelism comes from starting lanes early (warm-up / look-back) and PROVING, by bitwise state
 * comparison at the hand-off, that the lane had converged onto the sequential trajectory.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wm_dev.h"
#include "wm_exact.h"

#include "wm_k0_resample.h"
#include "wm_k0_spectrum.h"
#include "wm_k0_afc.h"
#include "wm_k0_power.h"
#include "wm_k0_activity.h"
#include "wm_k1_demod.h"
#include "wm_k2_common.h"
#include "wm_k2_clock.h"
#include "wm_k2_clock_sys.h"
#include "wm_k2_rla.h"

/* start[seg] must equal final[seg-1]; mismatching lanes are appended to `list`. */
/* heads: the launch that reads this list walks CHAINS (rla_lanes / clock_lanes / clock_sys_group with K2Args.bad): of a run of consecutive
 * listed segments only the first does anything there, the others return at once -- so only the first is listed (configs[2] listed 11 000
 * segments per context-push for 6 900 walks: 172 waves in the list launch instead of 108).
 * (Round 6 also measured the list in two parts -- the heads of runs of three or more segments in waves of their own: a long run is the
 * T1/C1 chain's framer inside a T1 / C1 telegram, whose chip clock is a PI loop with an integral that never resets there,
 * rtl_wmbus.c:790-796, so no speculative start inside the telegram can match: walks of up to 15 segments in configs[2], a quarter of that
 * chain's walks longer than three -- a clean signal with a third of the noise's edges per step.  No gain: the walk is 120 steps of 16
 * trips whatever shares its wave; removed.) */
__device__ __forceinline__ void k2_verify_lane(const WmPush &g, uint32_t algo, uint32_t lane, const uint32_t *st_start, const uint32_t *st_final, uint32_t words,
                                               uint32_t *list, uint32_t *n_list, uint32_t *bad, uint32_t heads)
{
    if (lane >= 2u * g.nseg[algo] * g.S) return;
    uint32_t ch, stream, seg;
    lane_decode(g, algo, lane, ch, stream, seg);
    if (!(g.flags & (ch ? WM_F_S1 : WM_F_T1C1)) || seg == 0) return;
    const uint64_t sidx = ((uint64_t)ch * g.S + stream) * g.nseg_cap[algo] + seg;
    const uint32_t *p = st_start + sidx * words, *q = st_final + (sidx - 1) * words;
    bool same = true;
    for (uint32_t k = 0; k < words; k++) same &= p[k] == q[k];
    /* the verdict per segment, laid out [chain][segment][capture] so that a wave's 64 captures store one line (capture-major it
     * was 200 000 scattered 4-byte stores per verification: read-modify-write traffic worth 2 ms of every step) */
    if (bad) bad[((uint64_t)ch * g.nseg_cap[algo] + seg) * g.S + stream] = same ? 0u : 1u;
    if (same) return;
    if (heads && bad && seg > 1u) {                      /* my predecessor's verdict, worked out here as its own thread does (segment 0 is never listed) */
        const uint32_t *pp = p - words, *qp = q - words;
        bool prev_same = true;
        for (uint32_t k = 0; k < words; k++) prev_same &= pp[k] == qp[k];
        if (!prev_same) return;                          /* inside a run: its head walks me */
    }
    list[atomicAdd(n_list, 1u)] = lane;
}

__global__ void k2_verify(WmPush g, uint32_t algo, const uint32_t *st_start, const uint32_t *st_final, uint32_t words,
                          uint32_t *list, uint32_t *n_list, uint32_t *bad, uint32_t heads)
{
    wm_framer_prio();
    k2_verify_lane(g, algo, blockIdx.x * blockDim.x + threadIdx.x, st_start, st_final, words, list, n_list, bad, heads);
}

/* The end of a push's framer stage in ONE launch (round 6: it was four): the last verification of either framer and the two
 * carries -- the end state of every row's last segment becomes the next push's start state.  (If a verification still lists
 * segments, wmbus_collect finishes them with the host in the loop and carries again.) */
struct K2Finish {
    const uint32_t *st_start[2], *st_final[2];           /* [framer] */
    uint32_t *list[2], *n_list[2], *bad[2], *carry[2];
    uint32_t words[2], verify[2], do_carry[2], heads[2];
};
__global__ void k2_finish(WmPush g, K2Finish f)
{
    wm_framer_prio();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t algo = 0; algo < 2u; algo++) {
        if (f.verify[algo]) k2_verify_lane(g, algo, t, f.st_start[algo], f.st_final[algo], f.words[algo], f.list[algo], f.n_list[algo], f.bad[algo], f.heads[algo]);
        if (f.do_carry[algo] && t < 2u * g.S)
            for (uint32_t k = 0; k < f.words[algo]; k++)
                f.carry[algo][(uint64_t)t * f.words[algo] + k] = f.st_final[algo][((uint64_t)t * g.nseg_cap[algo] + g.nseg[algo] - 1u) * f.words[algo] + k];
    }
}

#include "wm_k3_bursts.h"
#include "wm_k3_levels.h"
#include "wm_k3_repair.h"
#include "wm_k3_rescue.h"
#include "wm_k3_quality.h"
#include "wm_k_pair.h"
