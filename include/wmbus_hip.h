/*
 * wmbus_hip.h -- C ABI of libwmbus_hip.so, the MI355X (gfx950) back end for the rtl-wmbus
 * cu8 -> datagram hot path.
 *
 * The reference (xaelsouth/rtl-wmbus) has no library interface: its boundary is the process
 * (stdin cu8, argv switches, stdout lines) and, inside it, the per-sample loop of main()
 * (/root/reference/rtl_wmbus.c:1298-1357) that drives t1_c1_signal_chain (:1038-1116) and
 * s1_signal_chain (:1130-1208), which in turn call the packet decoders
 * (t1_c1_packet_decoder.h:649-712, s1_packet_decoder.h:233-282).  This header is the seam a
 * maintainer would bind instead of that loop; each entry point names what it replaces.
 * INTEGRATION.md shows the replacement main() and the ctypes binding.
 *
 * Plain C, plain pointers and sizes, no C++/torch types.  All functions return 0 on success or
 * a negative WMBUS_E* code; nothing in the library calls exit().  One context serves
 * `n_streams` independent captures that advance in lock step (same byte count per push).
 */
#ifndef WMBUS_HIP_H
#define WMBUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WMBUS_BLOCK_BYTES 4096u   /* the reference consumes stdin in 4096-byte units (rtl_wmbus.c:1249,1301) */
#define WMBUS_MAX_CHANNELS 8      /* channels of one wideband capture decoded by one context (cfg.input_channels) */

enum {
    WMBUS_OK = 0,
    WMBUS_EINVAL = -1,      /* bad argument / configuration                         */
    WMBUS_ENOMEM = -2,      /* host or device allocation failed                     */
    WMBUS_EDEVICE = -3,     /* HIP runtime error (see wmbus_last_error)             */
    WMBUS_EOVERFLOW = -4,   /* (no longer returned: exhausted chip / burst storage is a wmbus_timing.warnings bit) */
    WMBUS_ENODEVICE = -5    /* no HIP device: this library has no CPU fallback      */
};

enum { WMBUS_CHAIN_T1C1 = 0, WMBUS_CHAIN_S1 = 1 };
enum { WMBUS_ALGO_RLA = 0, WMBUS_ALGO_T2A = 1 };

/* Mirrors the reference's switches (rtl_wmbus.c:855-866, parsed at :892-967). */
typedef struct wmbus_cfg {
    unsigned decimation;        /* -d N, default 2                                   */
    int simultaneous;           /* -s                                                */
    int accurate_atan;          /* 1 unless -a                                       */
    int remove_dc;              /* -o                                                */
    int t1c1_enabled;           /* 0 after -p T                                      */
    int s1_enabled;             /* 0 after -p S                                      */
    int rla_enabled;            /* 0 after -r 0                                      */
    int time2_enabled;          /* 0 after -t 0                                      */
    int show_algorithm;         /* -v                                                */
    int fixed_timestamp;        /* 1: print "TS" instead of the wall clock (tests)   */
    /* batch geometry */
    unsigned n_streams;         /* independent captures processed per push           */
    int device;                 /* HIP device ordinal                                */
    size_t max_push_bytes;      /* capacity per stream per push, multiple of 4096    */
    /* tuning (0 = default) */
    unsigned seg_len;           /* clock-recovery time segment, decimated samples (power of two, 1024 ... 2^20); 0: 32768 -- 65536 for
                                   batches of >= 64 captures at decimation 2 with exact arithmetic and no -s, 16384 for batches of
                                   < 64 captures whose pushes are 2^15 ... 2^19 decimated samples (a live stream); with
                                   clock_waves = 1: 32768 / 16384 / 8192 by batch size */
    unsigned rla_seg_len;       /* run-length framer time segment                    */
    unsigned warmup_t1c1;       /* IIR warm-up before a segment, T1/C1 chain         */
    unsigned warmup_s1;         /* IIR warm-up before a segment, S1 chain            */
    unsigned rla_lookback;      /* speculative run-length lookback                   */
    unsigned host_threads;      /* host decoder threads, 0 = auto                    */
    int keep_taps;              /* 1: wmbus_read_tap may be used (the debug views of the last push).  0: no views -- the context then
                                   computes the RSSI only for the samples a packet decoder reads (the default switches at
                                   decimation 2 ... 5): same datagrams, fewer instructions */
    /* Low-pass in front of the decimator.  BOXCAR = the moving averages the reference's main()
     * runs (rtl_wmbus.c:1333-1344): what every reference binary computes, bit for bit.
     * POLYPHASE = lp_ppf_butter_1600kHz_160kHz_200kHz (rtl_wmbus.c:258-294 over ppf.h:46-59), which
     * the reference defines but never calls: an extension, 1.6 MS/s (decimation 2, no -s) only. */
    int prefilter;
    /* Discriminator arctangent: WMBUS_ATAN_LIBM = cargf / pi, what the reference is built with (atan2.h:7-10,
     * rtl_wmbus.c:523-529); WMBUS_ATAN_APPROX1 / 2 = atan2_approximation / atan2_approximation2 (atan2.h:14-74),
     * the alternatives its source keeps behind `#elif 0` / `#else`: extensions, ignored with -a. */
    int atan_mode;
    unsigned spill_words;       /* tuning: run-length chip spill arena, 32-bit words (0 = default) */
    /* Downstream conveniences, OFF by default (the drop-in prints exactly what the reference prints).  The two
     * framers work on every burst, so a clean telegram is printed twice (README.md:105-108): dedup_twins drops the
     * later of two lines of one capture and mode with the same payload from different framers that complete within one
     * longest-telegram time; only_crc_ok prints CRC-clean telegrams only (what e.g. wmbusmeters keeps). */
    int dedup_twins, only_crc_ok;
    /* 0 (default): off.  1: S1 RESCUE -- an S1 telegram of the time2 framer that the GPU's decoder, like the reference's, drops at the first
     * Manchester pair that reads 00 or 11, and whose chips lie whole inside the push, is decoded again on the GPU with every invalid pair
     * decided by its two soft symbols, by the fixed integer rule defined below under S1 RESCUE.  A telegram whose block CRCs are then all
     * clean is printed as a clean S1 line (CRC flag 1, wmbus_line.crc_ok = 1); every other line is the one of a context without the
     * field, in the same order, and every line comes with a rescue record (wmbus_rescue, wmbus_line_rescues() below).  The field switches
     * the level records of line_levels on by itself, as crc_repair and line_quality do.  0 is in every respect the context without this
     * field: the same kernels, buffers, bytes and lines.  WMBUS_EINVAL: anything above 1; together with bursts_to_host (nothing is
     * decoded on the GPU then), with s1_enabled = 0 or with time2_enabled = 0 (there is no subject then).  (The newest field: directly in
     * front of input_windows.  From line_quality to the end of the struct every field is pinned to its neighbours by the tests of
     * the features before this one; only_crc_ok / input_windows is a seam no test pins, and only fields behind it move, together.) */
    unsigned s1_rescue;
    unsigned input_windows;     /* 1 (default, also for 0): one device input window per stream; 2: two, used alternately, so
                                   that wmbus_stage() for the next push may run while the previous one is in flight (the
                                   copies run on their own HIP stream).  wmbus_device_input() names the window the next
                                   wmbus_process() will read. */
    /* 0 (default): off.  1: LINE QUALITY -- every datagram line comes with a quality record (wmbus_quality, wmbus_line_quality() below):
     * the transmitter's chip rate, the jitter of the decision instants and the eye opening of the soft symbols at them, measured on the
     * GPU by the fixed integer rule defined below under LINE QUALITY, for the telegrams of the time2 framer that the GPU decoded whole
     * inside a push (n = 0 for every other line).  The lines themselves do not change.  The field switches the level records of
     * line_levels on by itself, as line_power and crc_repair do.  0 is in every respect the context without this field: the same
     * kernels, buffers, bytes and lines.  WMBUS_EINVAL: anything above 1; together with bursts_to_host (nothing is decoded on the GPU
     * then: there is nothing it could measure).  (The newest field: directly in front of tolerance_mode -- every field from
     * tolerance_mode to the end of the struct is pinned to its neighbours by the tests of the features before this one, and
     * input_windows / tolerance_mode was the last seam no test pinned -- nothing else moves.) */
    unsigned line_quality;
    /* 0 (default): every soft symbol, RSSI byte and chip is bit-identical to the reference's.  1: TOLERANCE MODE for the
     * default switches (both chains, cargf arctangent, no -P): the discriminator uses a polynomial arctangent and the two
     * FIR low-passes fused multiply-adds, so soft symbols agree with the reference's to 2e-6 (absolute; they lie in
     * [-1, 1]) instead of bit for bit; RSSI, clock recovery and framers stay exact on those symbols.  A telegram whose
     * decision hangs on the last bits of a soft symbol may decode differently (DESIGN_HISTORY.md section 12 and DESIGN.md section 6 count them). */
    int tolerance_mode;
    /* 0 (default): off.  1: CRC REPAIR -- a telegram of the time2 framer that the GPU has decoded whole inside a push and that fails a block
     * CRC is repaired on the GPU by flipping its least reliable chips, by the fixed integer rule defined below under CRC REPAIR; a
     * repaired telegram is printed as if those chips had been received (CRC flag 1, wmbus_line.crc_ok = 1), every other line is the one
     * of a context without the field, and every line comes with a repair record (wmbus_repair, wmbus_line_repairs() below).  The field
     * switches the level records of line_levels on by itself, as line_power does (wmbus_line_levels works): the rule reads the soft
     * symbols and the preamble window they are measured on.  0 is in every respect the context without this field: the same kernels,
     * buffers, bytes and lines.  WMBUS_EINVAL: anything above 1; together with bursts_to_host (nothing is decoded on the GPU then: there
     * is nothing it could repair).  (The newest field: directly in front of rounds_on_host -- every field from there to the end of the struct is
     * pinned to its neighbours by the features before this one -- nothing behind it moves.) */
    unsigned crc_repair;
    /* Tuning and test knobs, 0 = the library's default.  (Rounds 1-4 read these from WMBUS_* environment variables inside the
     * push path; as configuration two contexts of one process can differ, and nothing in a push calls getenv.) */
    unsigned rounds_on_host;    /* 1: no hand-off rounds are enqueued unattended: every hand-off failure is finished by the host-driven
                                   path of wmbus_collect (wmbus_timing.slow_path); the GPU test suites run once with it */
    /* 0 (default): off.  1: CHANNEL ACTIVITY -- every collect comes with one record per burst of energy in each pipeline row's 200 kHz
     * channel, whether a framer locked on it or not (wmbus_burst, wmbus_activity() below): the census that answers "how much of what was
     * sent did I get?".  Made on the GPU from the timeline of CHANNEL POWER, in the integer arithmetic defined below under CHANNEL
     * ACTIVITY.  The field switches line_power's stage on by itself, as line_power switches the survey on (wmbus_line_power,
     * wmbus_read_channel_power work).  The lines do not change.  0 is in every respect the context without these two fields: the same
     * kernels, buffers and bytes.  Anything above 1 is WMBUS_EINVAL.
     * channel_activity_ratio_q8 = T: a level block is active where its power lies above T / 256 times the floor.  0: 1024 (x 4).  Any
     * other value outside 257 ... 65535, and a non-zero T without channel_activity, is WMBUS_EINVAL.  (The newest fields: in front of
     * the two RSSI knobs, which stay directly in front of line_power; nothing behind them moves.) */
    unsigned channel_activity;
    unsigned channel_activity_ratio_q8;
    unsigned rssi_full;         /* 1: the RSSI of every sample in the demodulation kernel even without debug views (A/B of RSSI on demand) */
    unsigned rssi_dense_pm;     /* RSSI on demand pauses for 16 pushes when more than this many per mille of a push's tiles were listed
                                   (0: 200; configs[2] lists 310 and is faster on the full pass) */
    /* 0 (default): off.  1: CHANNEL POWER -- every datagram line comes with a power record (wmbus_power, wmbus_line_power() below): the
     * signal in the telegram's 200 kHz channel, the noise floor in front of it and their ratio, measured on the GPU from the RAW input, in
     * front of every gain and independent of input_agc, in the integer arithmetic defined below under CHANNEL POWER.  The field switches
     * the survey on by itself, as input_afc does (wmbus_read_spectrum works), and the level records of line_levels, which carry every
     * line's access-code sample (wmbus_line_levels works).  The lines themselves do not change.  0 is in every respect the context
     * without this field: the same kernels, buffers and bytes.  Anything above 1 is WMBUS_EINVAL.  (Directly in front of bursts_to_host,
     * nothing behind it moves.) */
    unsigned line_power;
    unsigned bursts_to_host;    /* 1: every burst travels to the host packet decoders as chips (round 1's path) instead of being decoded
                                   on the GPU where it lies inside the push */
    /* 0 (default): the survey of input_spectrum / input_afc accumulates for ever (SPECTRUM below).  A = 1 ... 31: THE SURVEY FORGETS -- the
     * stream is cut into epochs of 2^A level blocks (2^A x 512 input samples) and the survey holds the current epoch and the one before
     * it, between 2^A + 1 and 2^(A+1) level blocks once the stream is that long: wmbus_read_spectrum returns that view and AFC locks on
     * it, so a transmitter that has gone silent, a receiver that drifts or one strong telegram heard once no longer hold the lock for
     * ever.  The definition is below under SPECTRUM AGE.  WMBUS_EINVAL: above 31; without input_spectrum or input_afc.  0 is in every
     * respect the context without this field: the same kernels, buffers and bytes.  (The newest fields, this one and the next: directly
     * in front of burst_caps, nothing behind them moves.) */
    unsigned input_spectrum_age;
    /* All 0 (default): every channel of input_channels is fixed at input_channel_hz[c].  Entry c non-zero: A LOCK PER CHANNEL -- channel c
     * of every capture carries an AFC state of its own and follows its transmitter within input_channel_hz[c] +- input_channel_afc_hz[c]
     * Hz, by AFC's rule on the capture's survey; the meters of two channels are different devices with different errors.  Any non-zero
     * entry switches the survey on by itself, as input_afc does; input_afc = 1 together with input_channels stays refused -- this array is
     * the switch of a channel list.  The contract is below under CHANNEL AFC; wmbus_read_input_afc() reads the lock of pipeline stream
     * capture x C + channel.  WMBUS_EINVAL: a non-zero entry at c >= input_channels (or without channels);
     * |input_channel_hz[c]| + input_channel_afc_hz[c] > Fin / 2; the array together with input_afc.  All 0 is in every respect the context
     * without this field: the same kernels, buffers and bytes. */
    unsigned input_channel_afc_hz[WMBUS_MAX_CHANNELS];
    unsigned burst_caps[4];     /* tests: burst storage {headers, chip words, packets, bytes} (0: sized from the batch), to reach the
                                   WMBUS_WARN_BURSTS_DROPPED paths */
    /* 0 (default): off.  1: AUTOMATIC FREQUENCY CORRECTION -- every capture of the context is shifted by an offset of its own, found on the
     * GPU from that capture's own survey (the max-hold spectrum of input_spectrum, which this field switches on by itself:
     * wmbus_read_spectrum works) and applied within the same push: the telegram that reveals the offset is decoded with it.  The
     * nominal is input_shift_hz; input_afc_range_hz says how far from it a transmitter may lie (0: 64000 -- the +-43.4 kHz of a +-50 ppm
     * dongle at 868 MHz, the bundled capture's own -10.3 kHz and a bin).  The arithmetic, the state carried from push to push and the
     * limits are defined below under AFC; wmbus_read_input_afc() reads the lock.  input_afc alone switches the conversion kernel on, as
     * a shift alone does.  WMBUS_EINVAL: input_afc above 1; together with input_channels (a channel list has input_channel_afc_hz instead);
     * |input_shift_hz| + range > Fin / 2; input_afc_range_hz without input_afc.  0 is in every respect the context without these two
     * fields: the same kernels, buffers and bytes.  (The newest fields: directly in front of k1_small_tile, nothing behind them moves.) */
    unsigned input_afc;
    unsigned input_afc_range_hz;
    unsigned k1_small_tile;    /* 1: the first pass of the demodulation kernel on 976-sample tiles even where the 2000-sample tile of
                                   512 threads is available (decimation 2, no -s, RSSI on demand); A/B */
    /* 0 (default): off.  1: CHANNEL SURVEY -- for every capture and every level block of 512 input samples the context computes a 512-point
     * windowed DFT of the raw input on the GPU, in the exact integer arithmetic defined below under SPECTRUM, and accumulates per capture
     * and bin the sum of the power and its maximum (max-hold) over all pushes; wmbus_read_spectrum() returns the arrays and
     * wmbus_spectrum_channels() turns them into a list of channels: where the transmitters of a capture are, before anything has decoded
     * -- the value input_shift_hz / input_channel_hz want.  The stage only reads the input: a context with the field prints the lines of
     * the same context without it, and a cu8 context at the native rate stays on the plain path (no conversion kernel).  0 is in every
     * respect the context without this field: the same kernels, buffers and bytes.  Anything above 1 is WMBUS_EINVAL.  (Directly in front
     * of input_channels.) */
    unsigned input_spectrum;
    /* 0 (default): one capture holds one channel.  C = 1 ... WMBUS_MAX_CHANNELS: every capture of the context is a wideband capture that is
     * decoded C times, channel c shifted by input_channel_hz[c] -- signed Hz with the meaning and the range of input_shift_hz below
     * (|f| <= Fin / 2); 0 Hz and duplicates are allowed.  The raw bytes are staged once per capture, the DC estimate and the AGC gain are
     * taken once per capture, in front of the rotation; the contract is below under CHANNELS.  input_shift_hz must be 0 with channels, C
     * above WMBUS_MAX_CHANNELS and a shift beyond Fin / 2 are WMBUS_EINVAL.  0 is in every respect the context without these two fields:
     * the same kernels, buffers and bytes.  (The newest fields: in front of
     * k1_tiles_per_block, so that every field from there on -- the input stage's among them -- keeps its place from the end of the struct.) */
    unsigned input_channels;
    int input_channel_hz[WMBUS_MAX_CHANNELS];
    unsigned k1_tiles_per_block;/* consecutive tiles a block of that first pass takes, each tile's input loaded while the one before
                                   is computed (0: the default; 1: one tile per block, no prefetch) */
    /* 0 (default): off.  1: PER-BLOCK AGC -- the input gain is found on the GPU, for every level block of 512 input samples from that
     * block's own peak, with the exact integer arithmetic defined below next to wmbus_read_input_gain(); it takes the place of
     * input_gain_q8, which must then be 0 or 256 (anything else together with input_agc is WMBUS_EINVAL, as is an input_agc above 1).
     * For captures whose level does not suit the pipeline's 8 bits -- a weak 16-bit or float capture, a weak cu8 / cs8 one, weak and strong
     * transmitters in one capture -- which otherwise decode nothing and give no hint why.  input_agc alone switches the conversion kernel
     * on, as a shift or the DC blocker alone does; 0 is in every respect the context without this field: the same kernels, buffers and
     * bytes.  (Placed in front of clock_waves; the fields behind it keep their order.) */
    unsigned input_agc;
    unsigned clock_waves;       /* how a clock-recovery lane group's filter cascade (iir.h:49-77 behind rtl_wmbus.c:1089-1111) is laid onto
                                   waves: 4 = systolic, the sections on the four waves of a block (round 6; 0: the default); 1 = one wave,
                                   software-pipelined across the sections (rounds 1-5).  Same records in memory, same datagrams; A/B */
    /* 0 (default): off.  1: every datagram line comes with a level record (wmbus_level, wmbus_line_levels() below): the frequency offset
     * and the deviation of its telegram, measured on the GPU from the soft symbols of the preamble in front of the access code, in the
     * integer arithmetic defined below under LINE LEVELS -- the feedback cfg.input_shift_hz needs.  The lines themselves do not change.
     * 0 is in every respect the context without this field: the same kernels, the same buffers, the same lines.  (In front
     * of the input stage's five, which close the struct.) */
    unsigned line_levels;
    /* 0 (default): the input is at decimation x 800 kHz, as the reference demands ("use a multiple of 800kHz", rtl_wmbus.c:1274-1292).
     * Otherwise the rate of the cu8 input in Hz (>= 800000): the context resamples it on the GPU to decimation x 800 kHz with the exact
     * integer polyphase filter of wmbus_resampler_design() and decodes that stream.  wmbus_stage / wmbus_device_input /
     * wmbus_process then take RAW bytes (max_push_bytes counts them); resampled bytes enter the pipeline in whole 4096-byte blocks,
     * the rest waits for the next push (a push that completes no block yields no lines) and is dropped at the end of the input, as
     * the reference drops a partial block.  wmbus_line.sample counts decimated samples of the resampled stream.  A rate equal to
     * decimation x 800 kHz is the same as 0. */
    unsigned input_rate_hz;
    /* 0 (default): the channel the pipeline expects (868.95 MHz, or 868.625 MHz with cfg.simultaneous) is the centre of the capture, as
     * the reference demands.  Otherwise the offset in Hz, signed, from the capture's centre to that channel: a capture tuned to 868.70 MHz
     * is decoded with input_shift_hz = 250000.  The context multiplies the input by e^(-j 2 pi f m / Fin) on the GPU -- inside the resampler
     * or the conversion kernel, where the samples are staged -- with the exact integer arithmetic defined below next to
     * wmbus_shift_design().  |f| <= Fin / 2, Fin = input_rate_hz (decimation x 800000 if 0).  A shift alone switches the conversion
     * kernel on: everything said below about raw bytes, whole blocks and the clip count then holds for a cu8 capture as well.  0 is in
     * every respect the context without this field. */
    int input_shift_hz;
    /* 0 (default): off.  R = 1 ... 12: the I/Q DC offset of the input (zero-IF receivers: HackRF, E4000 dongles, Pluto, Lime) is estimated
     * and subtracted on the GPU, per I and Q, in front of everything else that happens to a sample, with the exact integer arithmetic
     * defined below next to wmbus_read_input_dc(): a one-pole average over level blocks of 512 input samples, time constant 2^R blocks
     * (R = 6: 32768 input samples, 20 ms at 1.6 MS/s -- the value recommended for zero-IF receivers; it rests on synthetic captures and CPU
     * runs of the reference on the restated arithmetic only).  This is NOT the reference's -o (cfg.remove_dc), which removes the DC of the
     * discriminator's output, a frequency offset.  input_dc alone switches the conversion kernel on, as a shift alone does; 0 is in every
     * respect the context without this field.  Anything above 12 is WMBUS_EINVAL. */
    unsigned input_dc;
    /* Sample format of the input, WMBUS_FMT_* (0 = cu8, what an RTL-SDR delivers and the reference reads), and a linear input gain in
     * Q8, 1 ... 65535 = x 1/256 ... x 256 (0 means 256 = x 1).  The arithmetic is defined below, next to wmbus_resampler_design().
     * With a format other than cu8 or a gain other than x 1 the context converts on the GPU, inside the resampler where cfg.input_rate_hz
     * asks for one, else in a conversion kernel of its own; the semantics follow input_rate_hz: wmbus_stage / wmbus_device_input /
     * wmbus_process and max_push_bytes count RAW bytes (2, 2, 4, 8 per sample; still multiples of 4096), converted bytes enter the
     * pipeline in whole 4096-byte blocks, the rest waits for the next push, wmbus_line.sample counts decimated samples of the converted
     * stream.  cu8 with gain 0 or 256 at the native rate is the path it always was: no extra kernel, no extra buffer. */
    unsigned input_format;
    unsigned input_gain_q8;
} wmbus_cfg;

/* cs8: int8 I, Q (HackRF).  cs16: little-endian int16 I, Q (Airspy, SDRplay, SoapySDR).  cf32: little-endian IEEE float I, Q, full
 * scale +-1.0 (GNU Radio, SigMF). */
enum { WMBUS_FMT_CU8 = 0, WMBUS_FMT_CS8 = 1, WMBUS_FMT_CS16 = 2, WMBUS_FMT_CF32 = 3 };

enum { WMBUS_PREFILTER_BOXCAR = 0, WMBUS_PREFILTER_POLYPHASE = 1 };
enum { WMBUS_ATAN_LIBM = 0, WMBUS_ATAN_APPROX1 = 1, WMBUS_ATAN_APPROX2 = 2 };

typedef struct wmbus_ctx wmbus_ctx;

/* One datagram line as the reference prints it (t1_c1_packet_decoder.h:671-699,
 * s1_packet_decoder.h:248-269), plus the keys that define its place in stdout. */
typedef struct wmbus_line {
    uint32_t stream;            /* the capture */
    uint8_t  chain, algo, crc_ok;
    uint8_t  channel;           /* cfg.input_channels: the channel of the capture the line was decoded on; 0 without channels */
    uint64_t sample;            /* global decimated-sample index of the completing chip */
    uint32_t text_off, text_len;/* into the buffer returned by wmbus_lines_text()        */
} wmbus_line;

/* LINE LEVELS (cfg.line_levels = 1; tests/level_ref.py restates the arithmetic in numpy).  One record per line of wmbus_lines().
 *   s[m]   the soft symbol of decimated sample m of the line's chain: the FIR output wmbus_read_tap("dphi") shows, IN FRONT of the -o DC
 *          remover -- offset_hz is what -o removes -- and independent of -o, -a, -r, -t beyond the symbols themselves.  With
 *          cfg.tolerance_mode the levels are computed from THAT mode's soft symbols (within 2e-6 of the reference's), so they may differ
 *          by a unit from an exact context's.
 *   a      sync_sample: the global decimated-sample index of the access-code chip, the chip carrying the sync flag that started the
 *          decoder which printed the line.
 *   window [a - lo, a - hi), N = lo - hi samples.  T1/C1 chain: lo = 256, hi = 128 (16 chips of the alternating preamble, ending 16 chips
 *          in front of the 0x543D hit).  S1 chain: lo = 782, hi = 586 (N = 196, about 8 chips, ending 24 chips in front of the 0x547696
 *          hit).  a - lo < 0 (the window would begin before the stream's first sample): the record is invalid, n = 0, both values 0.
 *   q[m]   = clamp(rint(s[m] 2^20), -2^20, 2^20); the product is exact in f32, rint rounds half to even, NaN gives 0.
 *   sum    = sum of q;   mean = floor((2 sum + N) / (2 N));   adev = sum of |q - mean|                       (integers only)
 *   One unit of s is 400 kHz and 400000 / 2^20 = 3125 / 8192; both divisions floor, also for negative numerators:
 *   offset_hz = floor((sum 3125 + N 4096) / (N 8192)),   dev_hz = floor((adev 3125 + N 4096) / (N 8192)),   n = N.
 * dev_hz is a MEAN ABSOLUTE deviation over the band-limited preamble, not a peak deviation: a clean +-50 kHz preamble reads about 32 kHz.
 * Integer sums do not depend on the order of a reduction, nor on tile, block or push boundaries: the records do not depend on how the
 * input is cut into pushes (the context carries the last 782 soft symbols of every chain and capture from push to push). */
typedef struct wmbus_level {
    uint64_t sync_sample;
    int32_t  offset_hz;
    uint32_t dev_hz;
    uint32_t n;
    uint32_t pad;
} wmbus_level;

/* Per-push timings measured with HIP events on the library's own stream (ms). */
typedef struct wmbus_timing {
    float demod_ms;             /* front end + discriminator + FIR + RSSI kernel; with cfg.input_rate_hz also the resampler in front of it, with cfg.input_spectrum the survey
                                   (in a batch lane, wmbus_batch_lane_stats: this context's own launches -- its mate's follow on the same stream, in the mate's figure) */
    float clock_ms;             /* IIR clock recovery + time2 framer (incl. re-runs)  */
    float rla_ms;               /* run-length framer (incl. re-runs)                  */
    float gather_ms;            /* burst extraction (and, without debug views, the RSSI of the tiles the bursts touch; with cfg.line_levels the level kernels) */
    float d2h_ms;               /* burst copy to pinned host memory                   */
    float gpu_total_ms;         /* first kernel start -> last copy done               */
    float host_decode_ms;       /* packet decoders + formatting (wall clock)          */
    unsigned clock_reruns, rla_reruns, ema_retries;
    uint64_t chips[2][2];       /* chips produced in this push, [chain][algo]         */
    uint64_t bursts;            /* candidate bursts handed to the host decoders       */
    float turn_wait_ms;         /* host time spent waiting for this process's turn in the demodulation kernel */
    unsigned warnings;          /* WMBUS_WARN_* of this push (the push succeeded)     */
    unsigned slow_path;         /* 1: hand-off verification needed more rounds than run on the device unattended, or an
                                   RSSI value computed on demand could not be proven and the push took the full pass */
    float rssi_ms;              /* RSSI on demand: the launch over the listed tiles (part of gather_ms); 0 otherwise */
    unsigned rssi_mode;         /* WMBUS_RSSI_*: how this push got its RSSI */
    unsigned rssi_tiles;        /* RSSI on demand: (tile, capture) pairs listed in this push */
    unsigned clock_round[4], rla_round[4];   /* segments re-run in the unattended rounds, round by round (beyond the rounds enqueued: 0) */
    /* a context that resamples, shifts, removes the input's DC, levels it or converts (cfg.input_rate_hz, input_shift_hz, input_dc, input_agc, input_format, input_gain_q8): the cu8 bytes this push's input became,
     * all streams (whether the pipeline took them in this push or they wait for the next block to fill), and how many of them the
     * clamp to 0 ... 255 changed -- the feedback an input gain needs.  Both 0 on the plain cu8 path.  With cfg.input_channels both count
     * all channels of all captures. */
    uint64_t input_bytes_out, input_clipped;
} wmbus_timing;

/* wmbus_timing.rssi_mode.  EVERY_SAMPLE: in the demodulation kernel (contexts with debug views, option kernels, cfg.rssi_full).
 * ON_DEMAND: only where a packet decoder reads it.  PAUSED: an on-demand context whose bursts
 * cover most of its tiles takes the full pass for sixteen pushes.  FELL_BACK: a value read could not be proven, the push was
 * finished by the full pass (slow_path is set too). */
enum { WMBUS_RSSI_EVERY_SAMPLE = 0, WMBUS_RSSI_ON_DEMAND = 1, WMBUS_RSSI_PAUSED = 2, WMBUS_RSSI_FELL_BACK = 3 };

/* The reference never gives up on an input (rtl_wmbus.c:729-803 has no bound); neither does a push.  When an
 * interferer makes the run-length framer emit more chips than even the spill arena holds, or more candidate bursts
 * than the burst arena, the excess is dropped (datagrams inside it may be lost), all carried state stays exact. */
enum { WMBUS_WARN_CHIPS_DROPPED = 1, WMBUS_WARN_BURSTS_DROPPED = 2 };

/* Process-wide HIP runtime defaults this library wants, applied through the environment: GPU_MAX_HW_QUEUES=16 unless the
 * caller has set the variable (ROCm maps HIP streams onto 4 hardware queues by default and streams that share a queue
 * serialise: a batch of eight contexts runs at 55 % of its rate on four).  The runtime reads the variable ONCE, at the
 * first HIP call of the process, so this must run before that -- wmbus_batch_open() calls it, the CLI calls it first thing
 * in main(); an application that uses HIP before it opens a batch calls it (or exports the variable) itself.  The library
 * does nothing at load time.  WMBUS_KEEP_HW_QUEUES=1 in the environment turns the call into a no-op.  Not thread-safe
 * against concurrent getenv/setenv (it is a setenv): call it before starting threads. */
void wmbus_runtime_init(void);

void wmbus_default_cfg(wmbus_cfg *cfg);

/* Replaces the state set-up at rtl_wmbus.c:1249-1273,1296 (framer/decoder resets, LUT). */
int  wmbus_open(const wmbus_cfg *cfg, wmbus_ctx **out);
void wmbus_close(wmbus_ctx *ctx);
const char *wmbus_last_error(const wmbus_ctx *ctx);

/* Replaces fread() at rtl_wmbus.c:1301: copy `nbytes` (multiple of 4096) of stream `stream`
 * from host memory into the device input window of the next push (asynchronously, on the context's copy stream;
 * wmbus_process orders its kernels behind the copies). */
int  wmbus_stage(wmbus_ctx *ctx, unsigned stream, const uint8_t *cu8, size_t nbytes);
/* Page-locked host memory for wmbus_stage sources (hipHostMalloc): copies from it run at the PCIe
 * rate and asynchronously; any other host pointer works too, through the driver's bounce buffer. */
void *wmbus_alloc_pinned(size_t nbytes);
void  wmbus_free_pinned(void *p);
/* Same for HBM-resident producers: device address of the stream's input window.  With one input window (the default) the
 * window of a push in flight must stay untouched until wmbus_collect has returned: the rare slow paths of a push (a hand-off
 * repair, the full RSSI pass behind an unprovable on-demand value) read it again at collect time.  wmbus_stage enforces that;
 * a producer that writes through this pointer has to keep to it itself, or open the context with cfg.input_windows = 2. */
void *wmbus_device_input(wmbus_ctx *ctx, unsigned stream);

/* Replaces the sample loop rtl_wmbus.c:1310-1356 for `nbytes` staged bytes of every stream:
 * launches the kernels (asynchronously on the context's stream). */
int  wmbus_process(wmbus_ctx *ctx, size_t nbytes);
/* Waits for the push, runs the host packet decoders, makes the lines available.  Lines are in
 * the reference's stdout order within each stream, streams in ascending order. */
int  wmbus_collect(wmbus_ctx *ctx);

size_t wmbus_lines(const wmbus_ctx *ctx, const wmbus_line **lines);
const char *wmbus_lines_text(const wmbus_ctx *ctx, size_t *len);
/* The level records of the last push's lines: the same count and the same order as wmbus_lines() (cfg.dedup_twins / only_crc_ok drop a
 * level with its line).  A context opened without cfg.line_levels: 0, and *levels = NULL. */
size_t wmbus_line_levels(const wmbus_ctx *ctx, const wmbus_level **levels);

int  wmbus_get_timing(const wmbus_ctx *ctx, wmbus_timing *t);

/* Debug taps of the last push (requires cfg.keep_taps): what = "dphi" (f32), "rssi" (u8),
 * "bits" (u8 0/1).  Returns the number of elements written, or a negative error. */
long wmbus_read_tap(wmbus_ctx *ctx, const char *what, int chain, unsigned stream,
                    void *dst, size_t max_elems);
/* All chips of the last push for one stream/chain/algo as u32 words
 * [15:8] rssi, [7:0] value (bit0 data, bit1 sync, bit2 framer reset
 * before this chip); `pos` (optional) receives the global decimated-sample index per chip.  A context
 * opened without cfg.keep_taps computes the RSSI only where a packet decoder reads it: the rssi field is 0 then. */
long wmbus_read_chips(wmbus_ctx *ctx, int chain, int algo, unsigned stream,
                      uint32_t *dst, uint64_t *pos, size_t max_elems);

/* Device self-test of the exact scalar arithmetic the kernels use (correctly rounded sqrt and
 * divide, the restated glibc atan2f, the polar discriminator rtl_wmbus.c:517-534) on n operand
 * pairs: o_sqrt = sqrt(|a|), o_div = a/b, o_atan2 = atan2f(a, b),
 * o_disc[i] = discriminator(i=a[i], q=b[i], i'=b[i+1], q'=a[i+1]). */
int  wmbus_selftest_math(int device, const float *a, const float *b, float *o_sqrt, float *o_div,
                         float *o_atan2, float *o_disc, size_t n);

/* Device self-test of the demodulation kernel's two low-pass filters (fir.h:48-72 with the coefficients of
 * rtl_wmbus.c:369-391, lp_fir_butter_800kHz_100kHz_160kHz / _32kHz_36kHz) on one row: x[0 .. n + 48) holds 48 samples of history followed by the n inputs
 * (n a multiple of 4, at most 976: one tile of the kernel); out[0 .. n) receives the 11-tap filter's outputs, out[n .. 2n) the 46-tap one's. */
int  wmbus_selftest_fir(int device, const float *x, float *out, size_t n);

/* Device self-test of the run-length framer's integer divisions (the kernel's own functions: a truncated quotient through the
 * hardware's approximate reciprocal and a +-1 repair for dividends below 2^24 and divisors 4..4095, the integer divide
 * elsewhere), compared on the device with the compiler's division: every divisor 4..4095 with every multiple below 2^24 and
 * its two neighbours (3.5e8 cases), every divisor 1..8192 with the dividends 2^24 - 64 .. 2^24 + 64 and 0..128, each with
 * either sign.  Returns the number of wrong quotients (0 is the only good answer) or a negative error; first16 (optional,
 * 32 words) receives (dividend, divisor) of the first wrong ones, *cases (optional) the number of cases looked at. */
long long wmbus_selftest_udiv(int device, uint32_t *first16, unsigned long long *cases);

/* Measurement aid: the host half of wmbus_collect (sort, strip / format, merge: wm_decoder.c, replacing the decoders' fprintf at
 * t1_c1_packet_decoder.h:671-699 / s1_packet_decoder.h:248-269) over the records of the context's last push again, `reps` times, without
 * any GPU work.  Returns the lines of one repetition; *seconds receives the wall clock of all of them. */
long wmbus_debug_replay_decode(wmbus_ctx *ctx, unsigned reps, double *seconds);

/* SAMPLE FORMATS, GAIN AND RESAMPLER: the arithmetic (tests/format_ref.py and tests/resample_ref.py restate it in numpy).
 * Every format yields an int16 sample x per I and per Q, and a shift F:
 *     cu8   x = 2 u - 255                                                            F = 15
 *     cs8   x = 2 s + 1                       (the cu8 rule on s ^ 0x80)             F = 15
 *     cs16  x = s                                                                    F = 22
 *     cf32  x = clamp(rint(f * 32768), -32768, 32767), round half even, NaN -> 0     F = 22
 * With acc = the resampler's sum below (for an input already at decimation x 800 kHz: acc = 16384 * x[n]) and g = cfg.input_gain_q8
 * (256 if 0), the byte the pipeline gets is
 *     byte = clamp((acc * g + (128 << (F + 8))) >> (F + 8), 0, 255)                  (product in int64)
 * For cu8 with g = 256 that is (acc + 255 * 16384 + 16384) >> 15.  A cu8 byte u written as cs8 u - 128, as cs16 128 * (2 u - 255) or as
 * cf32 (2 u - 255) / 256 gives, at g = 256, the byte stream of the cu8 capture: byte = u at the native rate.  Integers only behind the
 * one rounding of cf32, so the bytes do not depend on tile, block or push boundaries.  |acc| <= 32768 * sum|taps| < 2^31 is checked
 * when a context with a 16-bit format is opened.
 *
 * The resampler behind cfg.input_rate_hz; host only, no device needed.  out_hz / in_hz = L / M in lowest terms (L <= 32, M <= 1024,
 * in_hz >= 800000, out_hz a multiple of 800000; else WMBUS_EINVAL).  taps (may be NULL: geometry only; cap = its int16 capacity,
 * >= L * T) receives L phases of T = 16 * max(1, ceil(M / L)) taps, taps[p * T + k]: a Kaiser-windowed sinc (beta 8, cut-off
 * 0.45 * min(in_hz, out_hz)) in Q14, every phase summing to exactly 16384.  With x = 2 * byte - 255 (0 before the stream starts),
 * output n of a stream is, for I and Q alike,
 *     acc  = sum over k < T of taps[((n * M) % L) * T + k] * x[floor(n * M / L) - k]
 *     byte = clamp((acc + 255 * 16384 + 16384) >> 15, 0, 255)
 * and exists once input floor(n * M / L) has been pushed: integers only, so the bytes do not depend on how the input is cut into pushes. */
int  wmbus_resampler_design(unsigned in_hz, unsigned out_hz, unsigned *L, unsigned *M, unsigned *T, int16_t *taps, size_t cap);
/* FREQUENCY SHIFT (cfg.input_shift_hz = f, signed Hz; tests/shift_ref.py restates it in numpy): input sample m of the stream (m counts
 * from the stream's first sample over all pushes, 64 bits) is multiplied by e^(-j 2 pi f m / Fin), Fin = cfg.input_rate_hz or
 * decimation x 800000, in integers:
 *     step  = floor((f * 2^32 + Fin / 2) / Fin) mod 2^32         (floor division, also for f < 0; 64-bit)
 *     phase = (step * m) mod 2^32                                (a function of m alone: nothing is accumulated across pushes)
 *     i     = ((phase + 2^21) mod 2^32) >> 22                    (10 bits, rounded; 1024 wraps to 0)
 *     c[i]  = rint(16384 cos(2 pi i / 1024)),  s[i] = rint(16384 sin(2 pi i / 1024))       (computed in double, stored as int16)
 *     yi = clamp((xi c + xq s + 8192) >> 14, -32768, 32767),  yq = clamp((xq c - xi s + 8192) >> 14, -32768, 32767)     (int32, >> floors)
 * With a shift cu8 and cs8 samples are 16 bits wide before the rotation, so that its rounding costs nothing: x = 64 (2 u - 255),
 * x = 64 (2 s + 1), F = 21 (|x| <= 16320, |x| sqrt 2 < 32768); cs16 and cf32 keep x and F = 22.  y takes the place of x in everything
 * above: the resampler's sum (history before the stream: y = 0; the history carried between pushes holds rotated samples) or
 * acc = 16384 y, then the gain and the clamp with that F.  |acc| <= 32768 * sum|taps| < 2^31 is checked for every format when a
 * context with a shift is opened.  Only integers follow the one rounding of cf32: the bytes do not depend on tile, block or push
 * boundaries.  Without a shift nothing changes.
 *
 * Host only, no device needed: the step, and (table may be NULL; cap = its int16 capacity, >= 2048) the 1024 entries {c[i], s[i]};
 * entry i + 256 is {-s[i], c[i]}.  WMBUS_EINVAL for |shift_hz| > in_hz / 2 or in_hz < 800000. */
int  wmbus_shift_design(unsigned in_hz, int shift_hz, uint32_t *step, int16_t *table, size_t cap);
/* CHANNELS (cfg.input_channels = C, cfg.input_channel_hz): several channels of one wideband capture in one context -- S1 at 868.30 MHz and
 * T1/C1 at 868.95 MHz from one Airspy / HackRF capture, each at its own centre.  No new arithmetic: channel c of capture k is decoded
 * EXACTLY as a context with input_shift_hz = input_channel_hz[c] and otherwise the same configuration decodes capture k -- the bytes handed
 * to the pipeline, the lines, the level records, chips and taps.  Format, rate, gain, input_dc and input_agc combine with channels as
 * they do with a shift; a 0 Hz channel goes through the rotating rule with step 0 (table entry 0 = {16384, 0}; cu8 / cs8 widened x 64,
 * F = 21), which gives exactly the bytes and the clip count of the unshifted rule.  The DC estimate and the AGC gain are taken in front
 * of the rotation: they are per capture and computed once, not per channel.
 *   pipeline width  S = n_streams x C; pipeline stream v = k C + c.  n_streams stays the context's captures.
 *   per capture     wmbus_stage, wmbus_device_input, max_push_bytes, the fill callback of a batch, wmbus_read_input_dc,
 *                   wmbus_read_input_gain: `stream` is the capture k.
 *   per pipeline stream   wmbus_read_resampled, wmbus_read_tap, wmbus_read_chips: `stream` is v.
 *   defaults        everything the library chooses by batch width (seg_len, storage sizes, RSSI on demand) takes S.
 *   lines           wmbus_line.stream is the capture, wmbus_line.channel the channel; captures ascending, within a capture channels
 *                   ascending, within a channel the reference's stdout order.  dedup_twins works per (capture, channel); the level
 *                   records follow the lines as they always do.
 *   timing          wmbus_timing.input_bytes_out and input_clipped count all channels.
 *   batch           wmbus_batch_* count captures and wmbus_batch_plan splits captures, as ever; each context carries all channels of its
 *                   captures; the sink's wmbus_line.stream is the batch-wide capture, with `channel` beside it. */
/* SPECTRUM (cfg.input_spectrum = 1; tests/spectrum_ref.py restates it in numpy and Python integers).  With x' the format's int16 sample per
 * I and Q by the UNSHIFTED rules above (cu8 2 u - 255, cs8 2 s + 1, cs16 s, cf32 as it is), behind the DC blocker where cfg.input_dc is
 * set (x' = clamp(x - dc[k]), the table of I/Q DC BLOCKER below), m the sample's index within the stream and level block k = m >> 9:
 *     v[n]  = 64 x'[512 k + n] for cu8 / cs8,  x'[512 k + n] for cs16 / cf32        n = 0 .. 511, per component (|v| <= 32768)
 *     w[n]  = (16384 - c[2 n] + 1) >> 1      c[i] = the cosine of the shift's 1024-entry table (wmbus_shift_design); 0 .. 16384, a Hann window in Q14
 *     y[n]  = (v[n] w[n] + 8192) >> 14                                              (>> floors; fits int16)
 *     z     = y in bit-reversed order (9 bits); then radix-2 decimation in time, stages s = 1 .. 9, half = 2^(s-1):
 *             for every group base g (multiple of 2^s) and j < half:  a = z[g + j], b = z[g + j + half], i = j (1024 >> s),
 *               t_re = (b_re c[i] + b_im s[i] + 8192) >> 14,   t_im = (b_im c[i] - b_re s[i] + 8192) >> 14       (products in int64, >> floors)
 *               z[g + j] = a + t,   z[g + j + half] = a - t                                                      (int32, nothing scaled, nothing clamped)
 *     pw[j] = (z_re[j]^2 + z_im[j]^2) >> 16        (uint64 product; < 2^32: |z| <= sum|y| <= 2^23.5)
 *     bin   b = (j + 256) mod 512  <->  f_b = (b - 256) Fin / 512,  Fin = cfg.input_rate_hz or decimation x 800000: ascending from -Fin / 2
 *     sum[b] += pw (uint64),   peak[b] = max(peak[b], pw) (uint32),   blocks += 1          per capture, over all pushes since open or the last reset
 * The twiddle multiply is the rotation rule of FREQUENCY SHIFT: t = b e^(-j 2 pi i / 1024) with the same table and the same rounding;
 * entries 0 and 256 multiply exactly, so no stage is special.  The butterfly graph and its roundings are the definition, the schedule is
 * not: any grouping of stages gives the same integers.  Sums and maxima of integers do not depend on the order of a reduction and a push
 * always holds whole level blocks, so the three arrays do not depend on tile, block or push boundaries.  The stage reads the RAW bytes of
 * the push at Fin: in front of the rotation, the resampler, the gain and the AGC, per capture (not per channel of cfg.input_channels).
 * sum would overflow after about 2^33 full-scale level blocks (a full-scale tone on a bin centre reaches pw = 2^31, a little more; 2^42 samples); the reset
 * is the remedy.
 *
 * wmbus_read_spectrum: the accumulators of one capture (`stream`), 512 entries each; any of sum / peak / blocks may be NULL.  To be called
 * when no push is in flight (after wmbus_collect).  reset != 0 zeroes that capture's accumulators behind the read.  Returns 512, or a
 * negative error: WMBUS_EINVAL on a context without cfg.input_spectrum.  It needs no cfg.keep_taps: it is feedback, like
 * wmbus_read_input_dc. */
long wmbus_read_spectrum(wmbus_ctx *ctx, unsigned stream, uint64_t *sum, uint32_t *peak, uint64_t *blocks, int reset);
/* SPECTRUM AGE (cfg.input_spectrum_age = A, 1 ... 31; tests/afc_age_ref.py restates it).  What SPECTRUM says about "all pushes since open
 * or the last reset", and the overflow of sum, describe the default A = 0.  With A set the survey forgets.  All captures of a context
 * advance in lock step: K is the context's index of a level block, counted from the stream's first sample over all pushes, 64 bits wide;
 * a reset does not restart it.  The epoch of level block K is e(K) = K >> A: E = 2^A level blocks per epoch.  After a push whose last
 * level block is K_last, with e_now = e(K_last), the VIEW of a capture is
 *     members  = the level blocks K <= K_last with e(K) in {e_now - 1, e_now} and K >= K_reset
 *     sum[b]   = sum of pw[K][b] over the members (uint64),   peak[b] = max of pw[K][b] over the members (uint32),   blocks = their number
 * with pw SPECTRUM's, unchanged, and K_reset = 0 or the level block behind the last wmbus_read_spectrum(reset) of that capture.  The view
 * holds between E + 1 and 2 E level blocks once the stream is that long; it is a function of the stream and of K_last alone -- not of how
 * the input was cut into pushes, nor of any grouping of level blocks on the GPU.  wmbus_read_spectrum returns the view (reset empties it),
 * and AFC evaluates its rule on the view: where AFC says "the accumulators as they stand now", read "the view".  sum cannot overflow:
 * it holds at most 2^32 level blocks of pw < 2^32.  wmbus_spectrum_channels takes arrays and is untouched.
 * What is left of the limit "the max-hold never forgets" with A set: a transmitter holds the lock for at most two epochs after its last
 * telegram, and a lock that has lost its transmitter stays where it is until another hit in range appears (the state stays, as AFC says).
 * A push that is longer than two epochs is surveyed by its last E + 1 ... 2 E level blocks only. */
/* The channels of a survey; host only, no device needed, intermediate integers 128 bits wide.  Defaults for 0: width_hz 200000,
 * min_ratio_q8 1024 (x 4), rel 8.  WMBUS_EINVAL for in_hz < 800000, blocks == 0 or 0 < min_ratio_q8 < 257.  Returns the hits written
 * (at most cap), strongest first:
 *     W   = clamp(floor(width_hz 512 / in_hz), 1, 256);   Fp = max(1, peak sorted ascending [255]);   Fm = max(1, (floor(sum[b] / blocks)) sorted ascending [255])
 *     B[b] = sum of peak[b .. b + W)  for b = 0 .. 512 - W;   all b alive
 *     repeat while hits < cap:  best = the alive b of the largest B (the lowest b on a tie);  stop if none, or B[best] 256 < min_ratio_q8 W Fp,
 *                               or (not the first hit and B[best] rel < B of the first hit)
 *        e[i] = max(0, peak[i] - Fp);  lo = best;  up to three times:  den = sum e[lo .. lo + W),  num = sum e[i] (i - 256) over the same i;
 *            cb = floor((2 num + den) / (2 den));  nlo = clamp(cb + 256 - W / 2, 0, 512 - W);  done if nlo == lo or this was the third time, else lo = nlo
 *        offset_hz = floor((2 num in_hz + 512 den) / (1024 den));   ratio_q8 = min(floor(B[best] 256 / (W Fp)), 2^32 - 1);   floor_peak = Fp, floor_mean = Fm
 *        every b with |b - best| < W dies
 * Every division floors, also for negative numerators.  den > 0 on the first trip follows from min_ratio_q8 > 256; a re-centred window
 * without any bin above the floor (den = 0) keeps the window before it.  offset_hz has the sign and the meaning of cfg.input_shift_hz:
 * it is the value to pass there.  The reference level is the median of the MAX-HOLD (telegrams are millisecond bursts: a mean over seconds
 * dilutes them away), so the threshold does not move with the length of the capture.  What the defaults rest on, and what the rule cannot
 * do: rel and the x 4 rest on four captures only -- the bundled 1.6 MS/s RTL-SDR capture (mixed by -43 ... +200 kHz: one hit each, within
 * 1.2 bins), the synthetic three-channel 4.0 MS/s capture of the channels tests (three hits) and cu8 noise of sigma 1 ... 30 counts (none;
 * strongest window x 1.1 of the floor).  A transmitter more than rel times weaker than the strongest hit is not reported: it cannot be
 * told from the strongest hit's skirts (13 ... 17 dB below their carrier on those captures).  A zero-IF receiver's DC spike is a peak at
 * 0 Hz unless cfg.input_dc removes it. */
typedef struct wmbus_channel_hit { int32_t offset_hz; uint32_t ratio_q8; uint32_t floor_peak, floor_mean; } wmbus_channel_hit;
int wmbus_spectrum_channels(unsigned in_hz, const uint64_t *sum, const uint32_t *peak, uint64_t blocks,
                            unsigned width_hz, unsigned min_ratio_q8, unsigned rel, wmbus_channel_hit *out, unsigned cap);
/* AFC (cfg.input_afc = 1, cfg.input_afc_range_hz = range, 0: 64000; the nominal is cfg.input_shift_hz; tests/afc_ref.py restates it in
 * Python integers).  Per capture, carried from push to push: held_hz (int32, initially the nominal), locked (0), changes (0),
 * ratio_q8 (0), base (uint32 phase, 0).  For every push of n_in input samples, after the survey has added this push's level blocks to
 * the capture's accumulators (SPECTRUM above):
 *     hits   = wmbus_spectrum_channels(Fin, sum, peak, blocks, 0, 0, 0, ..., cap = 8): the rule above with its defaults, strongest
 *              first, on the accumulators as they stand now, this push included
 *     cand   = the first hit with |offset_hz - nominal| <= range;  none: the state stays
 *     fold cand in if locked == 0 or |cand.offset_hz - held_hz| > floor(Fin / 256):
 *              held_hz = cand.offset_hz, ratio_q8 = cand.ratio_q8, locked = 1, changes += 1;  otherwise the state stays
 *     step   = floor((held_hz 2^32 + Fin / 2) / Fin) mod 2^32                        (wmbus_shift_design's rule)
 *     input sample j of this push (j = 0 .. n_in - 1) is rotated by the table entry of phase (base + step j) mod 2^32
 *     base'  = (base + step n_in) mod 2^32
 * Everything else of FREQUENCY SHIFT is unchanged: the index rounding, the table, the widening x 64 of cu8 / cs8 with F = 21, the clamp.
 * floor(Fin / 256) is two survey bins: the rule's own scatter on the four mixes of the bundled capture is at most 1.2 bins (SPECTRUM),
 * and a re-estimate inside that scatter must not move the shift.  Consequences:
 *   - while held_hz has had one value since the stream's first sample, base = step m and the bytes are exactly those of a context with
 *     input_shift_hz = held_hz;
 *   - before a lock the rotation runs with the nominal's step; for nominal 0 that is step 0, table entry {16384, 0}: exactly the bytes
 *     and the clip count of the unshifted rule, as the 0 Hz channel of CHANNELS;
 *   - the phase is continuous across a change, the frequency is not;
 *   - the resampler's carried history holds samples as they were rotated then;
 *   - the DC blocker, the AGC, the gain, the formats and the resampler combine with AFC as they do with a shift.
 * The limits:
 *   - the result depends on how the input is cut into pushes -- the first feature of this library of which that is true (a host that
 *     set input_shift_hz between pushes would have the same property);
 *     (cfg.crc_repair is the second: which telegrams it examines depends on the cut, CRC REPAIR below; cfg.line_quality the third, for
 *     the same reason: LINE QUALITY below)
 *   - a telegram that straddles a change is rotated with two frequencies;
 *   - telegrams in pushes before the first lock are decoded at the nominal;
 *   - the max-hold never forgets: wmbus_read_spectrum(reset) is the remedy on a long live stream;
 *     (that is the default, cfg.input_spectrum_age = 0; with the field set the survey holds the last two epochs: SPECTRUM AGE above)
 *   - one offset per capture: the strongest transmitter in range wins.
 *     (a channel list has a lock per channel instead, cfg.input_channel_afc_hz: CHANNEL AFC below)
 *
 * wmbus_read_input_afc: the state the last push of capture `stream` was rotated with (before the first push: the initial state).  To
 * be called when no push is in flight (after wmbus_collect).  It needs no cfg.keep_taps, like wmbus_read_input_dc.  Returns 0, or a
 * negative error: WMBUS_EINVAL on a context without cfg.input_afc. */
/* CHANNEL AFC (cfg.input_channel_afc_hz[c] = range of channel c, 0: the channel is fixed; tests/afc_age_ref.py restates it as a loop over
 * AFC's rule).  There is no new arithmetic.  What AFC says about "one offset per capture: the strongest transmitter in range wins" and
 * the refusal of input_afc with input_channels describe the per-capture switch; with the array set:
 *   - pipeline stream v = k C + c (capture k, channel c) carries an AFC state of its own: held_hz starts at input_channel_hz[c]; locked,
 *     changes, ratio_q8 and base at 0;
 *   - after the survey of a push AFC's rule runs once per v, on capture k's survey (with cfg.input_spectrum_age: on its view), with
 *     nominal = input_channel_hz[c] and range = input_channel_afc_hz[c];
 *   - a channel with range 0 skips the search: its step is that of input_channel_hz[c] and its base runs on -- exactly the bytes of the
 *     fixed channel of CHANNELS; wmbus_read_input_afc reads {input_channel_hz[c], 0, 0, 0} for it;
 *   - channel c of capture k is byte for byte, line for line and state for state what a single-channel context produces on capture k
 *     with input_shift_hz = input_channel_hz[c], input_afc = 1, input_afc_range_hz = input_channel_afc_hz[c], the same
 *     input_spectrum_age, the same pushes and otherwise the same configuration;
 *   - the DC estimate, the AGC gain and the survey stay per capture, taken once;
 *   - on such a context the `stream` of wmbus_read_input_afc is v.
 * Two channels may lock on the same transmitter (ranges may overlap; a hit is not used up).  SPECTRUM's limit carries over: a transmitter
 * more than rel (8) times weaker than the capture's strongest hit is not reported, whichever channel it lies in, so its channel never
 * locks and stays at its nominal.  AFC's other limits hold per channel: the cut into pushes, a telegram that straddles a change, the
 * pushes before the first lock; there is no switch per channel other than the range, and nothing tracks within a push. */
typedef struct wmbus_afc { int32_t shift_hz; uint32_t locked, changes, ratio_q8; } wmbus_afc;
long wmbus_read_input_afc(wmbus_ctx *ctx, unsigned stream, wmbus_afc *out);
/* CHANNEL POWER (cfg.line_power = 1; tests/power_ref.py restates it in numpy and Python integers on top of tests/spectrum_ref.py).  Integers
 * only; every division floors.  With pw[K][b] SPECTRUM's power of level block K (the stream's index of the block, counted from the
 * stream's first sample over all pushes, 64 bits) and bin b (ascending from -Fin / 2):
 *   band rows (the waterfall)   bp[K][j] = min(sum of pw[K][b] over b in [16 j, 16 j + 16), 2^32 - 1),  j = 0 .. 31: one row of 32 uint32
 *                               per capture and level block, each band Fin / 32 wide
 *   channel window              W  = clamp(floor(200000 x 512 / Fin), 1, 256), the survey's default window
 *                               nb = min(32, ceil(W / 16) + 1): one band more than the window needs, so that a window of W bins fits at
 *                               any alignment and nb is a constant of the context
 *   centre of pipeline row r = chain x S + v (chain WMBUS_CHAIN_*, v the pipeline stream of CHANNELS, S their number):
 *                               f_r = the frequency the stage kernel of THIS push rotates stream v by -- cfg.input_shift_hz,
 *                               cfg.input_channel_hz[c], or under AFC / CHANNEL AFC the held_hz the push was rotated with -- and with
 *                               cfg.simultaneous + 325000 for the T1/C1 chain, - 325000 for the S1 chain (the demodulation kernel's own
 *                               shift: it takes T1/C1 from above the centre)
 *                               cb = 256 + floor((1024 f_r + Fin) / (2 Fin)),   lo = clamp(cb - W / 2, 0, 512 - W)   (W / 2 floors),
 *                               j0 = min(lo >> 4, 32 - nb)
 *   channel power               P[r][K] = min(sum of bp[K][j0 .. j0 + nb), 2^32 - 1)
 *   line record                 for a line with access-code sample a (wmbus_level.sync_sample) and completing sample e
 *                               (wmbus_line.sample), both decimated samples:  m(n) = floor(n D M / L) with D the decimation and L / M
 *                               the resampler's ratio (1 / 1 without one);  ka = m(a) >> 9,  ke = m(e) >> 9
 *       signal blocks           ka < K < ke, whole level blocks strictly inside the telegram (the pipeline's filter delay, a few tens of
 *                               samples, is ignored).  number = their count;  n_signal = min(number, 65535);
 *                               signal = floor(sum of P / number)  (the count itself, not the capped field)
 *       noise blocks            K in [ka - G - Nn, ka - G) with K >= 0;  G = ceil(Fin / 51200), 10 ms, the longest preamble;
 *                               Nn = ceil(Fin / 25600), 20 ms.  number = their count;  n_noise = min(number, 65535);
 *                               noise = the element at index floor(number / 4) of their P sorted ascending: the lower quartile -- other
 *                               telegrams inside the window do not lift it
 *       ratio_q8                = min(floor(signal x 256 / noise), 2^32 - 1);  0 when n_signal or n_noise is 0;  for noise = 0:
 *                               2^32 - 1 when signal > 0, else 0
 *       first_block             = ka
 * The two clamps are guards no input reaches: the pw of all 512 bins of a level block add up to 512 x sum |y|^2 >> 16, at most 0.75 x 2^32.
 * P is a ratio's raw material, not a physical unit: signal and noise are in the survey's units of pw (SPECTRUM), summed over nb bands
 * (nb / 32 of the capture's bandwidth).  Sums of integers do not depend on the order of a reduction and a push always holds whole level
 * blocks, so rows, P and the records do not depend on how the input is cut into pushes: the context keeps, per row, P of the last
 * Nn + G + ceil(0.15 Fin / 512) level blocks in front of the current push (an S1 telegram of L = 255 lasts about 142 ms), so a level
 * block K < 0 is the only missing one.  The survey reads the raw bytes of a push, the pipeline may hold back a partial 4096-byte block
 * of converted bytes: P is always at or ahead of the lines.  The one exception is AFC, as in AFC's own contract: the window follows the
 * lock push by push, so P (and a record whose blocks straddle a change) depends on the cut there.  With cfg.input_spectrum_age every level
 * block of a push still gets its row; only the survey's accumulators skip old epochs.
 *
 * wmbus_line_power: the power records of the last push's lines, the same count and the same order as wmbus_lines() (cfg.dedup_twins /
 * only_crc_ok drop a record with its line).  A context opened without cfg.line_power: 0, and *power = NULL.
 * wmbus_read_waterfall: the band rows of the last push of one capture, 32 uint32 per level block into rows[0 .. 32 x cap_rows);
 * *first_block (may be NULL) receives the stream's index of the first row.  Returns the rows written.
 * wmbus_read_channel_power: P of the last push of pipeline row chain x S + stream_v into p[0 .. cap); *first_block as above.  Returns the
 * values written.  Both reads are to be called when no push is in flight (after wmbus_collect), need no cfg.keep_taps and return
 * WMBUS_EINVAL on a context without cfg.line_power.
 * wmbus_line_power_rule: the line record above from a timeline; host only, no device needed.  p[0 .. n) holds P of level blocks
 * first_block .. first_block + n - 1; a level block outside the array counts as missing, like K < 0.  WMBUS_EINVAL for in_hz < 800000 or
 * NULL pointers (p may be NULL for n = 0).
 * wmbus_line_power_block: m(sample) >> 9 for a context of that decimation and input rate (0: decimation x 800000); host only.
 * WMBUS_EINVAL where wmbus_resampler_design refuses the rate. */
typedef struct wmbus_power { uint64_t first_block; uint32_t signal, noise, ratio_q8; uint16_t n_signal, n_noise; } wmbus_power;
size_t wmbus_line_power(const wmbus_ctx *ctx, const wmbus_power **power);
long wmbus_read_waterfall(wmbus_ctx *ctx, unsigned capture, uint32_t *rows, uint64_t *first_block, size_t cap_rows);
long wmbus_read_channel_power(wmbus_ctx *ctx, int chain, unsigned stream_v, uint32_t *p, uint64_t *first_block, size_t cap);
int  wmbus_line_power_rule(const uint32_t *p, uint64_t first_block, size_t n, uint64_t ka, uint64_t ke, unsigned in_hz, wmbus_power *out);
int  wmbus_line_power_block(unsigned decimation, unsigned input_rate_hz, uint64_t sample, uint64_t *block);
/* CHANNEL ACTIVITY (cfg.channel_activity = 1; tests/activity_ref.py restates it in Python integers on top of tests/power_ref.py).  Integers
 * only; every division floors.  For every pipeline row r = chain x S + v on its own, with P[K] = CHANNEL POWER's P[r][K] and K counted
 * from the stream's first sample, T = cfg.channel_activity_ratio_q8 (0: 1024):
 *   epoch        e(K) = K >> 6, 64 level blocks.  q[e] = the element at index 16 of the epoch's 64 values of P sorted ascending (the lower
 *                quartile: telegrams inside the epoch do not lift it).  It exists once the epoch is complete
 *   floor        H = min(63, ceil(0.16 Fin / 32768) + 1) (9 at 1.6 MS/s);  floor[e] = min of q[e'] over max(0, e - H) <= e' <= e.  The
 *                window is longer than the longest telegram: an epoch that lies wholly inside an S1 telegram does not lift the floor
 *   active       act[K] = (P[K] x 256 > T x floor[e(K)]), products in 64 bits
 *   burst        a maximal run of active level blocks of length >= 2, evaluated when the epoch that holds the first inactive block behind
 *                it is complete:  first_block;  blocks;  mean = floor(sum of P / blocks), the sum in 64 bits;  floor = the floor of the
 *                epoch the run began in;  stream (the capture), channel and chain of the row
 *   not evaluated  a run of one block is dropped.  The stream's last incomplete epoch is never evaluated (as the reference drops a partial
 *                block): a burst whose closing block lies in it is not reported, and wmbus_close reports nothing more
 *   carrier      a carrier that never ends closes by itself: once all H + 1 epochs of the floor hold it, the floor is the carrier's own
 *                level and no block lies T / 256 above it.  One long record, then silence until the carrier goes: the rule's behaviour
 * The records of a stream, concatenated over its collects, are a function of the stream alone and do not depend on how the input is cut
 * into pushes -- the row's state (the incomplete epoch's P, the last H quartiles, the epoch count, the open run) stays on the GPU and moves
 * on once per push.  The one exception is AFC's, as in CHANNEL POWER: P itself follows the lock push by push.
 * What the rule rests on (measured with the restatement): synthetic captures of 2^19 samples, 40 frames/s, sigma 3, amplitudes 60, 8 and
 * 5: every frame found, both ends within one level block, nothing else reported.  cu8 noise of sigma 1, 3 and 30, 2048 level blocks each:
 * no record at x 4 or x 2, the largest P at most 1.88 x its lower quartile.  The bundled 1.6 MS/s capture: two records, (first_block,
 * blocks) = (748, 21) and (1424, 46), its two telegrams; at x 2 the same capture gives 76 records, real-world noise excursions, hence the
 * default of x 4.  The bundled 2.4 MS/s capture with cfg.simultaneous: one record (143, 33) on the T1/C1 row, none on the S1 row.  The
 * default rests on these two captures and on synthetic noise only; a site with impulsive interference may want a higher T.
 *
 * wmbus_activity: the records the last collect delivered, rows ascending (chain, then capture, then channel), first_block ascending within
 * a row.  A context opened without cfg.channel_activity, or a collect that closed no burst: 0, and *records = NULL.
 * wmbus_activity_progress (beyond the rule: what a caller needs to know when a burst can no longer get a line): the level blocks of the
 * stream the collects so far have taken in; every burst that closed in an epoch complete by then has been delivered.  0 without the field.
 * wmbus_activity_rule: the rule above over one row's whole timeline p[0 .. n) from level block 0; host only, no device needed.  Writes at
 * most cap records (stream, channel and chain 0) and returns the number found.  WMBUS_EINVAL for in_hz < 800000, a ratio_q8 that
 * cfg.channel_activity_ratio_q8 would refuse, or NULL pointers (p may be NULL for n = 0, out for cap = 0).
 * wmbus_activity_match: host only.  A line matches a burst of its row when its access-code level block ka -- wmbus_line_power_block of
 * wmbus_level.sync_sample -- satisfies first_block - 1 <= ka < first_block + blocks; the - 1 covers rates at which the preamble is shorter
 * than a level block.  Bursts of a row are separated by at least one inactive block, so these intervals are disjoint.  Returns the index
 * of the matching record among records[0 .. n) for the row (stream, channel, chain), or -1. */
typedef struct wmbus_burst { uint64_t first_block; uint32_t blocks, mean, floor; uint32_t stream; uint8_t channel, chain; uint8_t pad[2]; } wmbus_burst;
size_t wmbus_activity(const wmbus_ctx *ctx, const wmbus_burst **records);
uint64_t wmbus_activity_progress(const wmbus_ctx *ctx);
long wmbus_activity_rule(const uint32_t *p, size_t n, unsigned in_hz, unsigned ratio_q8, wmbus_burst *out, size_t cap);
long wmbus_activity_match(const wmbus_burst *records, size_t n, unsigned stream, unsigned channel, int chain, uint64_t ka);
/* CRC REPAIR (cfg.crc_repair = 1; tests/repair_ref.py restates it in numpy and Python integers on top of tests/telegram_ref.py and
 * tests/level_ref.py).  Integers only behind LINE LEVELS' rint.
 *   subject      a burst of the TIME2 framer (WMBUS_ALGO_T2A) that the GPU has decoded whole inside the push that holds its access code,
 *                whose decoder completed the telegram, whose CRC verdict is 0 and whose length L (air bytes, CRC bytes included) is at
 *                least 12.  Nothing else is examined: not the lines of the run-length framer (its chips record the end of a run, not a
 *                decision instant: the soft symbol there says nothing about the chip), not a burst cut by the end of a push and finished
 *                by the host decoders, not a decoder that gave up.  An S1 telegram with an invalid Manchester pair never completes, so
 *                S1 is repaired only where BOTH chips of a pair are wrong.
 *   chips        j = 0 is the access-code chip.  Byte b of the telegram holds the chips j = 1 + 12 b ... 12 + 12 b (T1),
 *                17 + 8 b ... 24 + 8 b (C1), 1 + 16 b ... 16 + 16 b (S1).  For chip j: p[j] its decimated sample, s the soft symbol there
 *                (LINE LEVELS' s: in front of -o; with cfg.tolerance_mode that mode's symbols), q[j] = LINE LEVELS' clamp(rint(s 2^20),
 *                -2^20, 2^20), c = LINE LEVELS' mean over the telegram's preamble window, 0 where that record is invalid (n = 0).  The
 *                reliability of the chip is r[j] = |q[j] - c|.
 *   blocks       the CRC blocks of the L air bytes: frame A 12 bytes, then blocks of 18; frame B blocks of 128; the last block is as
 *                long as what is left.  A bad block of fewer than 3 bytes cannot be repaired.
 *   candidates   of a bad block: the chips of its bytes, except those of the telegram's byte 0, the L-field (a flip there would change
 *                the length).  K = min(8, their number); the K candidates with the smallest (r, j), ascending; bit i of a pattern m is
 *                the i-th of them.
 *   patterns     m = 1 ... 2^K - 1: flip the chips of m and decode the block's bytes by the mode's code.  m is valid if every
 *                3-out-of-6 symbol (T1) or Manchester pair (S1) of the block is a code word and the block's CRC equals the CRC-16 of the
 *                bytes before it.  C1 is NRZ: every chip pattern is a code word, the CRC alone decides.  w(m) = sum of r over the flipped
 *                chips (64 bits).  The repair of the block is the valid m with the smallest (w, m); none valid: the block stays bad.
 *   telegram     repaired only if EVERY bad block has a repair.  Then its bytes are the repaired bytes, its line is formatted as if the
 *                GPU had decoded those chips -- CRC flag 1, the 3-out-of-6 flag recomputed over the whole telegram -- and
 *                wmbus_line.crc_ok = 1.  Otherwise line and bytes are exactly those of crc_repair = 0.  cfg.dedup_twins and
 *                cfg.only_crc_ok act behind the repair.
 *   record       one wmbus_repair per line, the count and the order of wmbus_lines() as for the level records.  All zero for a clean
 *                line and for a line that was no subject.  A subject that stayed bad reports blocks_bad and the repairs found for single
 *                blocks (blocks_repaired < blocks_bad), its line unchanged.  weight = sum of w over the repaired blocks, below 2^29
 *                (17 blocks of 8 chips of at most 2^21).
 * Only integers follow rint and a minimum over patterns does not depend on the order of a reduction, so the result for a subject depends
 * on the stream alone.  The limit, beside AFC's: WHICH telegrams are subjects depends on how the input is cut into pushes -- a telegram
 * that straddles a push edge is finished by the host decoders and is not repaired.
 * What a repair is worth.  A T1 or S1 pattern has to pass the line code AND the CRC; a C1 pattern only the CRC: an unrepairable C1 block
 * has at most 255 chances in 65 536 of matching by accident.  K = 8 and the rule rest on three captures and nothing else: the bundled
 * 1.6 MS/s capture (its second telegram, 117 air bytes, one invalid symbol in the last block: one chip flipped, weight 24 800, the
 * telegram the capture otherwise yields only when re-run 10.29 kHz lower) and two synthetic captures of 60 telegrams each near the
 * discriminator's threshold (T1 and C1 frame A; tests/golden/repair.json holds the counts), on which every repaired telegram equals the
 * bytes that were sent.  The errors of an FM discriminator near threshold come in clicks, not in single chips: most bad telegrams stay
 * bad.  Nobody has measured the rule on a capture with interference.
 *
 * wmbus_line_repairs: the repair records of the last push's lines, the same count and the same order as wmbus_lines() (cfg.dedup_twins /
 * only_crc_ok drop a record with its line).  A context opened without cfg.crc_repair: 0, and *records = NULL. */
typedef struct wmbus_repair { uint16_t blocks_bad, blocks_repaired, chips_flipped, pad; uint32_t weight; } wmbus_repair;
size_t wmbus_line_repairs(const wmbus_ctx *ctx, const wmbus_repair **records);
/* S1 RESCUE (cfg.s1_rescue = 1; tests/rescue_ref.py restates it in numpy and Python integers on top of tests/telegram_ref.py and
 * tests/level_ref.py).  Integers only behind LINE LEVELS' rint.
 *   subject      a packet record of the burst kernel that
 *                  - is an abort (the decoder gave up), of the TIME2 framer (WMBUS_ALGO_T2A), of the S1 chain;
 *                  - has a length: all eight pairs of the L-field were valid, and 12 <= L <= 292 (air bytes, CRC bytes included);
 *                  - with n = 1 + 16 L: all n chips, the access-code chip j = 0 included, lie whole inside this push's chip stream (CRC
 *                    REPAIR's test);
 *                  - was a Manchester violation and nothing else: data pair i = 0, 1, ... is the chips 1 + 2 i and 2 + 2 i, i_b the first
 *                    pair whose two hard chips are equal, and the decoder consumed exactly 2 i_b + 3 chips;
 *                  - would otherwise have come through: no chip 1 ... n - 1 carries the framer-reset marker, and the RSSI byte of every
 *                    chip 1 ... n - 2 is at least 5 (the chip that completes the telegram is exempt, as in the decoder).
 *                Nothing else is examined: not the run-length framer's bursts, not a burst cut by the end of a push (the host decoders
 *                finish or abort it), not an abort inside the L-field (the length is unknown then), not an RSSI or reset abort.
 *   decision     a valid pair keeps its hard value: 01 -> 1, 10 -> 0.  For an invalid pair, q_a and q_b are LINE LEVELS' quantised soft
 *                symbols clamp(rint(s 2^20), -2^20, 2^20) at the samples of its first and second chip (CRC REPAIR's row): the bit is 1 if
 *                q_b > q_a, 0 if q_b < q_a, and 0 on a tie.  The chip with the larger soft symbol is the 1: the maximum-likelihood
 *                decision for a Manchester pair, which needs no threshold and no preamble mean.  The pair's margin is |q_b - q_a|.
 *   verdict      the L bytes are assembled from the decided bits (first pair of a byte in its most significant bit) and the frame-A
 *                block CRCs are checked: 12 bytes, then blocks of 18, the last as long as what is left (a block of one byte is bad).
 *                The telegram is rescued only if EVERY block is clean; a subject with a bad block gives no line, exactly as without the
 *                field.  No chip is flipped on top of this: CRC REPAIR keeps its own subjects.
 *   line         of a rescued telegram: an S1 line with CRC flag 1, the first RSSI byte that of chip 1 (as the abort recorded it), the
 *                second that of chip n - 1, completed (timestamp, wmbus_line.sample) at the sample of chip n - 1; wmbus_line.crc_ok = 1.
 *                The decoder's bookkeeping does not change: it still was busy for 2 i_b + 3 chips only, so every access code it took
 *                without the field it takes with it, and every other line of the push is byte for byte the same.  A rescued line is
 *                sorted among the others by its completing sample; cfg.dedup_twins and cfg.only_crc_ok act behind the rescue (the
 *                run-length framer's line of the same telegram is its twin).
 *   record       one wmbus_rescue per line, the count and the order of wmbus_lines().  All zero for every line that is not a rescue.
 *                For a rescued line: status 1, pairs = the invalid pairs decided, min_margin = the smallest margin among them (LINE
 *                LEVELS' unit, at most 2^21), blocks = the CRC blocks of the telegram.  The records of subjects that gave no line (status
 *                2: a bad block; 3: rescued, but the push's byte storage was full) are only counted: wmbus_rescue_stats().
 * Only integers follow rint, so a subject's record depends on the stream alone.  The limits.  WHICH telegrams are subjects depends on how
 * the input is cut into pushes, as for CRC REPAIR.  An invalid pair inside the L-field stays an abort.  The RSSI gate is respected.  The
 * rule rests on two synthetic S1 captures near the discriminator's threshold (tests/golden/rescue.json holds the counts), on which every
 * rescued telegram equals the bytes that were sent; the bundled captures hold no S1 telegram that aborts this way, and nobody has
 * measured the rule on a real S1 capture or under interference.
 *
 * wmbus_line_rescues: the rescue records of the last push's lines, the same count and the same order as wmbus_lines() (cfg.dedup_twins /
 * only_crc_ok drop a record with its line).  A context opened without cfg.s1_rescue: 0, and *records = NULL.
 * wmbus_rescue_stats: of the last collect, the subjects a decoder took (status 1, 2 or 3 on a record that passed the busy test) and how
 * many of them gave a line (status 1).  Either pointer may be NULL.  Returns 0, or WMBUS_EINVAL without a context or without the field. */
typedef struct wmbus_rescue { uint16_t status, pairs; uint32_t min_margin; uint16_t blocks, pad; } wmbus_rescue;
size_t wmbus_line_rescues(const wmbus_ctx *ctx, const wmbus_rescue **records);
int wmbus_rescue_stats(const wmbus_ctx *ctx, unsigned *subjects, unsigned *rescued);
/* LINE QUALITY (cfg.line_quality = 1; tests/quality_ref.py restates it in Python integers on top of tests/repair_ref.py and
 * tests/level_ref.py).  Integers only behind LINE LEVELS' rint; floor(a / b) floors for negative a too.
 *   subject      a packet record of the burst kernel that is complete (WM_PKT_DONE), of the TIME2 framer (WMBUS_ALGO_T2A), with a length
 *                L (air bytes, CRC bytes included) of at most 292, whose n = off + cpb L chips lie whole inside this push's chip stream:
 *                the chips count from the access-code chip j = 0, off = 1, 17, 1 and cpb = 12, 8, 16 for T1, C1, S1 (CRC REPAIR's chips).
 *                These are CRC REPAIR's subjects without "not CRC-clean" and "L >= 12".  Everything else gets the all-zero record,
 *                n = 0: the lines of the run-length framer (its chips mark the end of a run, not a decision instant), a burst cut by a
 *                push edge and finished by the host decoders, a decoder that gave up.
 *   chips        pos[j] the push-relative decimated sample of chip j, v[j] its value, p[j] = pos[j] - pos[0].  The record is invalid
 *                (all zero) too if n < 2, if p[n-1] >= 2^17, if num <= 0 below, or if one of the two chip values does not occur.
 *   timing       64-bit integers.  With n <= 1 + 16 x 292 = 4673 and p < 2^17 every intermediate stays below 2^63: the largest is
 *                80 000 000 den, about 2.7 10^18.
 *                  j' = 2 j - (n - 1);  num = sum j' p[j];  den = sum j'^2 = n (n^2 - 1) / 3
 *                  chip_rate_chz = floor((80 000 000 den + num) / (2 num))
 *                the least-squares chip rate in hundredths of a chip per second (800 kHz den / (2 num), rounded): T1 / C1 nominal is
 *                10 000 000, S1 3 276 800.  (A framer decides at most one chip per sample, so p[j] >= j, num >= den / 2 and the figure is at
 *                most 80 000 000.)
 *                  B = floor((4 x 65536 num + den) / (2 den))          samples per chip in Q16
 *                  s = sum (65536 p[j] - B j);  A = floor((2 s + n) / (2 n))
 *                  e = sum |65536 p[j] - B j - A|
 *                  jitter_ns = floor((1250 e + 32768 n) / (65536 n))
 *                the mean absolute distance of a decision instant from the fitted clock; one decimated sample is 1250 ns.  Positions are
 *                whole samples: a perfect clock that does not sit on the sample grid reads a few hundred ns, not 0.
 *   eye          q[j] = LINE LEVELS' quantised soft symbol at pos[j], of the row CRC REPAIR reads (in front of -o; with
 *                cfg.tolerance_mode that mode's symbols).  n1, n0 the chips of value 1 and 0, S1, S0 the sums of their q (64 bits:
 *                4673 x 2^20 exceeds 2^31).
 *                  m1 = floor((2 S1 + n1) / (2 n1)), m0 likewise;  mid = floor((m1 + m0) / 2)
 *                  spread = sum |q[j] - m(v[j])|;  sigma = +1 if m1 >= m0, else -1
 *                  margin of chip j = sigma (q[j] - mid) for v[j] = 1, sigma (mid - q[j]) for v[j] = 0;  eye = the smallest margin
 *                and with hz(x, N) = floor((3125 x + 4096 N) / (8192 N)), LINE LEVELS' unit:
 *                  hi_hz = hz(m1, 1), lo_hz = hz(m0, 1), spread_hz = hz(spread, n), eye_hz = hz(eye, 1)
 *                eye_hz <= 0: a chip lies on the wrong side of the midpoint -- the direct cause of a bad CRC block.
 * The record is measured on the chips as received: cfg.crc_repair does not change it (a repair flips chips in its own copy).  Integer
 * sums do not depend on the order of a reduction, so a subject's record depends on the stream alone.  The limit, CRC REPAIR's: WHICH
 * telegrams are subjects depends on how the input is cut into pushes -- a telegram that straddles a push edge has n = 0.
 * The bundled 1.6 MS/s capture: its T1 telegram of 48 air bytes reads 99 800.14 chip/s, 1367 ns, hi 41 642, lo -68 343, eye 32 214 Hz; the
 * one of 117 bytes that fails its CRC 99 765.30 chip/s, 775 ns, eye -9 951 Hz: closed.
 *
 * wmbus_line_quality: the quality records of the last push's lines, the same count and the same order as wmbus_lines() (cfg.dedup_twins /
 * only_crc_ok drop a record with its line).  A context opened without cfg.line_quality: 0, and *records = NULL. */
typedef struct wmbus_quality {
    uint32_t n, chip_rate_chz, jitter_ns;
    int32_t  hi_hz, lo_hz;
    uint32_t spread_hz;
    int32_t  eye_hz;
    uint32_t pad;
} wmbus_quality;   /* 32 bytes */
size_t wmbus_line_quality(const wmbus_ctx *ctx, const wmbus_quality **records);
/* I/Q DC BLOCKER (cfg.input_dc = R, 1 ... 12; tests/dc_ref.py restates it in numpy).  With x the format's int16 sample per I and per Q
 * by the UNSHIFTED rules above (cu8 2 u - 255, cs8 2 s + 1, cs16 s, cf32 as it is), m the sample's index within the stream (64 bits) and
 * level block k = m >> 9 (512 input samples):
 *     S[k]  = sum of x over block k                                              (per I and Q; |S| <= 2^24)
 *     A[0]  = S[0] << R;   A[k] = A[k-1] - (A[k-1] >> R) + S[k]                  (int64; >> floors, also for A < 0)
 *     dc[k] = clamp((A[k] + (1 << (8 + R))) >> (9 + R), -32768, 32767)
 *     x'    = clamp(x - dc[k], -32768, 32767)
 * x' takes the place of x in everything above: the x 64 widening of cu8 / cs8 under a shift (|x'| <= 510: 64 x' still fits), the
 * rotation, the resampler's sum or acc = 16384 x', the gain, the clamp and the clip count.  The resampler's carried history holds x'
 * (rotated where there is a shift); history before the stream is 0.  A push is a multiple of 4096 raw bytes = 2048 / 2048 / 1024 / 512
 * samples, so it always holds whole level blocks.  dc[k] includes block k itself: nothing is delayed.  Only integers follow the one
 * rounding of cf32: the bytes do not depend on tile, block or push boundaries.  The time constant is 2^R blocks.
 *
 * Debug read (requires a context with cfg.input_dc, not cfg.keep_taps: it is the offset's feedback, as wmbus_timing.input_clipped is the
 * gain's): {dc_I, dc_Q} of every level block of the last push for one stream, in units of x.  Returns the number of pairs written, or a
 * negative error. */
long wmbus_read_input_dc(wmbus_ctx *ctx, unsigned stream, int16_t *iq, size_t cap_pairs);
/* PER-BLOCK AGC (cfg.input_agc = 1; tests/agc_ref.py restates it in numpy).  With x' the format's int16 sample behind the DC blocker
 * where cfg.input_dc is set (else x, by the UNSHIFTED rules above), m the sample's index within the stream and level block k = m >> 9
 * (the blocker's block of 512 input samples):
 *     P[k] = max over block k of (|x'_I| + |x'_Q|)                                (0 ... 65536)
 *     U    = 9 for cu8 / cs8, 16 for cs16 / cf32                                  (with or without a shift: the x 64 widening of the 8-bit
 *                                                                                  formats cancels against F = 21)
 *     g[k] = clamp(floor((96 << U) / max(P[k], 1)), 1, 65535)                     (uint32 division; 96 << 16 < 2^32)
 * g[k] takes the place of cfg.input_gain_q8 in the output rule: the byte of an output whose NEWEST input sample lies in block k (at the
 * native rate: the sample itself; behind the resampler: input floor(n M / L) of output n) is
 *     clamp((acc g[k] + (128 << (F + 8))) >> (F + 8), 0, 255),  the product in int64, F as above (15 / 22; 21 / 22 under a shift).
 * So the block's peak lands on +-96 of the byte's +-127: |I| + |Q| bounds either component after any rotation, and the resampler's
 * pass-band ripple and the gain's floor stay inside the rest.  Only integers follow the one rounding of cf32 and g[k] depends on block k
 * alone -- nothing is carried, there is no attack and no release: FSK has a constant envelope, a block's own peak is the estimate, and
 * an envelope that decays over several blocks loses weak telegrams behind strong ones -- so the bytes do not depend
 * on tile, block or push boundaries; a push always holds whole level blocks.  Consequences:
 *   - every block is brought to the same level, so the rssi a line prints is RELATIVE under AGC: it no longer tells a strong
 *     transmitter from a weak one;
 *   - a silent block is amplified up to the clamp of g: all-128 cu8 (x = 1, P = 2, g = 24576) gives the constant byte 176, all-zero
 *     cs16 the byte 128 -- constants, which the discriminator does not see;
 *   - behind the resampler an output's sum reaches back T - 1 samples, across a block edge too: a few outputs behind a strong-to-weak
 *     edge carry the strong block's samples under the weak block's gain and may clip; wmbus_timing.input_clipped counts them.
 *
 * Debug read (requires a context with cfg.input_agc, not cfg.keep_taps): g[k] of every level block of the last push for one stream.
 * Returns the number of values written, or a negative error. */
long wmbus_read_input_gain(wmbus_ctx *ctx, unsigned stream, uint16_t *g, size_t cap);
/* Debug read (requires cfg.keep_taps and a context that resamples, converts, shifts, removes the input's DC or levels it:
 * cfg.input_rate_hz, input_shift_hz, input_dc, input_agc, input_format, input_gain_q8): the
 * cu8 bytes the last push handed to the pipeline for one stream.  Returns the number of bytes written (0 for a push that completed no
 * block), or a negative error. */
long wmbus_read_resampled(wmbus_ctx *ctx, unsigned stream, uint8_t *out, size_t cap);
/* Pushes of this context that launched the resampler or the conversion kernel (0 for ever on the plain cu8 path, which a context
 * with cfg.input_shift_hz = 0, cfg.input_dc = 0, cfg.input_agc = 0 and nothing else set is). */
unsigned long long wmbus_resampler_launches(const wmbus_ctx *ctx);

/* Number of visible HIP devices (0 if none). */
int  wmbus_device_count(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Many captures on one device.  The reference is one stream per process (rtl_wmbus.c:1298-1356 IS its product); a
 * batch is `cfg->n_streams` of those loops side by side.  The library splits the captures over several receiver
 * contexts (default: 8, whole 64-capture groups each), drives every context on its own thread through the same
 * stage / process / collect steps as above, and overlaps them: one context's demodulation kernel runs beside the other
 * contexts' framer kernels and host decoding, and a context's next push is already on the GPU while its previous one
 * is decoded on the host.  This is what `rtl_wmbus_hip FILE...` and bench.py run.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct wmbus_batch wmbus_batch;

typedef struct wmbus_batch_io {
    /* SOURCE.  fill != NULL (needs cfg.input_windows = 2): called on a worker thread whenever streams
     * [first_stream, first_stream + n_streams) need their next push.  Write the bytes of stream s at
     * slab + (s - first_stream) * pitch (page-locked memory, `cap` bytes per stream) and return the byte count EVERY
     * stream of the group advances by (a multiple of 4096, <= cap; pad ended streams with no signal), or 0 when
     * the group's input has ended.  The bytes are RAW bytes of cfg.input_format; no signal is the byte 128 for cu8, 0 for cs8 and
     * cs16, 0.0f (all bytes 0) for cf32.  Calls for different groups may run concurrently.
     * fill == NULL: the input is resident in the device windows (wmbus_batch_stage / wmbus_batch_device_input):
     * every context makes `passes` pushes of `resident_bytes`. */
    size_t (*fill)(void *user, unsigned first_stream, unsigned n_streams, uint8_t *slab, size_t pitch, size_t cap);
    /* SINK (optional).  The lines of one push of one group, in the reference's stdout order per stream
     * (wmbus_line.stream counts within the whole batch); calls are serialised, a push's lines leave as a unit. */
    void (*lines)(void *user, unsigned first_stream, unsigned n_streams, const wmbus_line *lines, size_t n_lines,
                  const char *text, const wmbus_timing *timing);
    void *user;
    size_t resident_bytes;
    unsigned passes;
    /* 1: `fill` stages the group's bytes itself with wmbus_batch_stage() from page-locked memory of its own (slab is
     * NULL then): no host-side copy between the source and the PCIe transfer. */
    unsigned self_staged;
} wmbus_batch_io;

typedef struct wmbus_batch_stats {
    uint64_t samples;           /* input IQ samples consumed, all streams (raw bytes / bytes per sample of cfg.input_format) */
    uint64_t lines;             /* datagram lines produced                       */
    double   seconds;           /* wall clock of wmbus_batch_run                 */
    unsigned pushes;            /* context pushes                                */
    unsigned warnings;          /* WMBUS_WARN_* seen                             */
} wmbus_batch_stats;

/* cfg->n_streams = all captures of the batch; contexts = 0: the default split.  On failure *out still holds an
 * object whose wmbus_batch_last_error() explains; close it. */
int  wmbus_batch_open(const wmbus_cfg *cfg, unsigned contexts, wmbus_batch **out);
/* The split wmbus_batch_open would make, without opening anything (no device needed): returns the number of contexts and
 * writes the captures of each into counts[0 .. min(contexts, cap)). */
unsigned wmbus_batch_plan(const wmbus_cfg *cfg, unsigned contexts, unsigned *counts, unsigned cap);
void wmbus_batch_close(wmbus_batch *b);
const char *wmbus_batch_last_error(const wmbus_batch *b);
unsigned wmbus_batch_contexts(const wmbus_batch *b);
/* Context i and the streams it serves (its own wmbus_lines / wmbus_get_timing / taps describe its last push). */
wmbus_ctx *wmbus_batch_context(wmbus_batch *b, unsigned i, unsigned *first_stream, unsigned *n_streams);
/* wmbus_stage / wmbus_device_input by batch-wide stream number. */
int  wmbus_batch_stage(wmbus_batch *b, unsigned stream, const uint8_t *cu8, size_t nbytes);
void *wmbus_batch_device_input(wmbus_batch *b, unsigned stream);
/* Runs until every group's source has ended (or `passes` pushes per context).  Returns 0 or the first error. */
int  wmbus_batch_run(wmbus_batch *b, const wmbus_batch_io *io, wmbus_batch_stats *stats);
/* Lanes.  With fewer hardware queues than contexts (GPU_MAX_HW_QUEUES as the caller has it; HIP's own default is 4) neighbouring
 * contexts share a lane: one worker thread, one stream, and the latency-bound framer and burst kernels of the two leave as ONE launch
 * (streams that share a queue would run their pushes one after the other).  A lane holds two contexts at most; with a queue per
 * context every context is its own lane.  WMBUS_BATCH_LANES=N in the environment, read by wmbus_batch_open, overrides the count.
 * *lanes: the lanes of this batch; *paired_launches / *single_launches: kernel launches of the last wmbus_batch_run that carried two
 * contexts / one.  Any pointer may be NULL.  Returns 0, or WMBUS_EINVAL for a batch that is not open. */
int  wmbus_batch_lane_stats(const wmbus_batch *b, unsigned *lanes, unsigned long long *paired_launches, unsigned long long *single_launches);
/* For the SINK of a batch opened with cfg.line_levels: the level records of the lines the `lines` callback has just been handed, in
 * their order.  Valid only during that callback, with the first_stream it was called with (the group's context is decoding nothing else
 * meanwhile and the calls are serialised: no race).  Returns the count; 0 with *levels = NULL for any other first_stream or without
 * cfg.line_levels. */
size_t wmbus_batch_line_levels(const wmbus_batch *b, unsigned first_stream, const wmbus_level **levels);
/* The same for a batch opened with cfg.line_power: the power records of the lines the `lines` callback has just been handed. */
size_t wmbus_batch_line_power(const wmbus_batch *b, unsigned first_stream, const wmbus_power **power);
/* The same for a batch opened with cfg.channel_activity: the bursts of the collect whose lines the `lines` callback has just been handed;
 * wmbus_burst.stream counts from first_stream. */
size_t wmbus_batch_activity(const wmbus_batch *b, unsigned first_stream, const wmbus_burst **records);
/* The same for a batch opened with cfg.crc_repair: the repair records of the lines the `lines` callback has just been handed. */
size_t wmbus_batch_line_repairs(const wmbus_batch *b, unsigned first_stream, const wmbus_repair **records);
/* The same for a batch opened with cfg.line_quality: the quality records of the lines the `lines` callback has just been handed. */
size_t wmbus_batch_line_quality(const wmbus_batch *b, unsigned first_stream, const wmbus_quality **records);
/* The same for a batch opened with cfg.s1_rescue: the rescue records of the lines the `lines` callback has just been handed. */
size_t wmbus_batch_line_rescues(const wmbus_batch *b, unsigned first_stream, const wmbus_rescue **records);

#ifdef __cplusplus
}
#endif
#endif /* WMBUS_HIP_H */
