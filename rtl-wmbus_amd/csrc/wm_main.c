/*
 * wm_main.c -- `rtl_wmbus_hip`: drop-in for the reference's command line.
 *
 *   rtl_sdr -f 868.95M -s 1600000 - 2>/dev/null | rtl_wmbus_hip [-o] [-a] [-d N] [-p T|S] [-r 0] [-t 0] [-v] [-s] [-f] [-V]
 *
 * Same switches, usage text layout, exit codes and stdout line format as
 * /root/reference/rtl_wmbus.c:869-967,1217-1372; the per-sample loop (:1298-1357) is replaced by
 * wmbus_stage()/wmbus_process()/wmbus_collect() from libwmbus_hip.so.  Plain C; the GPU is only
 * reached through the C ABI in include/wmbus_hip.h.
 * Extensions (letters the reference does not use): -B bytes per GPU push, -L ms (a live stream's bytes never wait longer
 * than this for their push to fill; wm_reader.c), -G HIP device(s), -P polyphase pre-filter, -A 1|2 fast arctangents,
 * -I sample format of the input and -g input gain in dB or auto (converted on the GPU), -C I/Q DC blocker of the input, -w channel survey of the
 * input (a max-hold spectrum taken on the GPU: where the transmitters are, printed to stderr as a ready-made -O), -O auto[:Hz] that offset
 * found and applied on the GPU within the same run, per capture (auto:Hz entries inside an -O list: per channel), -E seconds a survey
 * that forgets, so that the lock follows the last seconds of a live stream, -l frequency offset and
 * deviation of every telegram appended to its line, -U / -W de-duplication, -T host:port (cu8 over TCP; the role of the reference's unused net_support.h:15-44 /
 * rtl_wmbus.c:1281), -S statistics, and
 *   rtl_wmbus_hip [switches] a.cu8 b.cu8 ...      batch mode: one capture per file, lines prefixed "a.cu8: ".
 * A batch is a wmbus_batch of the library per device: the files are split over several receiver contexts (whole groups
 * of 64, eight contexts at most) that run on their own threads and overlap each other, 2 MiB per file and push, the next
 * push read into page-locked memory and staged into a context's second input window while the previous one is in
 * flight.  With -G all (or -G 0,2,5) the files are sharded over the GPUs of the node, file i on device list[i mod n]
 * (file-per-GPU, no collective), each file's lines in its own order.  -M prints that map and exits.
 */
#include <arpa/inet.h>
#include <math.h>
#include <netdb.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <time.h>

#include "wm_reader.h"
#include "wmbus_hip.h"

#define VERSION "rtl_wmbus_hip 0.4 (MI355X/gfx950 back end)"
#ifndef COMMIT
#define COMMIT "unknown"          /* the Makefile passes the repository's HEAD, like the reference's does (Makefile:16,38) */
#endif

static void print_usage(const char *prog)
{
    fprintf(stdout, "rtl_wmbus: " VERSION "\n\n");
    fprintf(stdout, "Usage %s:\n", prog);
    fprintf(stdout, "\t-o remove DC offset\n");
    fprintf(stdout, "\t-a accelerate (use an inaccurate atan version)\n");
    fprintf(stdout, "\t-r 0 to disable run length algorithm\n");
    fprintf(stdout, "\t-t 0 to disable time2 algorithm\n");
    fprintf(stdout, "\t-d 2 set decimation rate to 2 (defaults to 2 if omitted)\n");
    fprintf(stdout, "\t   (this back end decimates by 1 ... 16: -d 17 and beyond, which the reference accepts, are refused)\n");
    fprintf(stdout, "\t-v show used algorithm in the output\n");
    fprintf(stdout, "\t-V show version\n");
    fprintf(stdout, "\t-s receive S1 and T1/C1 datagrams simultaneously. rtl_sdr _MUST_ be set to 868.625MHz (-f 868.625M)\n");
    fprintf(stdout, "\t-p [T,S] to disable processing T1/C1 or S1 mode\n");
    fprintf(stdout, "\t-f exit if flow of incoming data stops\n");
    fprintf(stdout, "\t-R rate of the input in samples/s when it is not -d x 800 kHz (2048000, 2.048M, 2048k): resampled on the GPU to -d x 800 kHz\n");
    fprintf(stdout, "\t   (output rate / input rate = L / M in lowest terms with L <= 32, M <= 1024; at least 800k; with -P only to 1.6 MS/s)\n");
    fprintf(stdout, "\t-I cu8|cs8|cs16|cf32 sample format of the input (default cu8; cs16 and cf32 little-endian, cf32 full scale +-1.0): converted on the GPU\n");
    fprintf(stdout, "\t-g dB input gain applied with that conversion, -48.2 ... 48.2 (a weak 16-bit capture wants 20 ... 40; -S prints the clipped share)\n");
    fprintf(stdout, "\t-g auto the gain found on the GPU, per block of 512 input samples from the block's own peak (weak and mixed-level captures; not together with -g dB; the rssi of a line is then relative)\n");
    fprintf(stdout, "\t-O Hz offset of the channel from the centre of the capture, signed (250k, -0.1M; rtl_sdr -f 868.70M wants -O 250k): shifted on the GPU, at most half the input rate\n");
    fprintf(stdout, "\t   a list (-O 325k,-325k; up to %d entries) decodes that many channels of one wideband capture at once and appends ;<channel Hz> to every line\n", WMBUS_MAX_CHANNELS);
    fprintf(stdout, "\t   -O auto finds the offset on the GPU, per capture, from the capture's own spectrum, within +-64 kHz of the centre (a +-50 ppm dongle), and applies it from the push\n");
    fprintf(stdout, "\t   that reveals it; -O auto:250k searches around 250 kHz instead.  With -v every change of the lock goes to stderr (afc: <Hz> Hz x<strength> over the floor;\n");
    fprintf(stdout, "\t   batch mode: per file, at the end).  The result depends on how the input is cut into pushes (-B)\n");
    fprintf(stdout, "\t   in a list an entry spelled auto:Hz follows its transmitter within +-64 kHz of Hz, each channel with a lock of its own (-O auto:325k,auto:-325k; -O auto:325k,-325k\n");
    fprintf(stdout, "\t   keeps the second fixed); -v prints afc[<channel Hz>]: <Hz> Hz x<strength> over the floor.  A bare auto inside a list is not taken\n");
    fprintf(stdout, "\t-C R remove the I/Q DC offset of the input, time constant 2^R x 512 samples, R = 1 ... 12; 6 suits zero-IF receivers (HackRF, E4000, Pluto, Lime)\n");
    fprintf(stdout, "\t-l append ;offset_hz;dev_hz to every line: frequency offset (what -O should add) and mean absolute deviation of the telegram's preamble, measured on the GPU; empty where the preamble lies before the stream\n");
    fprintf(stdout, "\t-n append ;signal;noise;x<strength> to every line (behind -l's fields, in front of a channel's): the power in the telegram's 200 kHz channel, the noise floor in the 20 ms in front of its preamble and their ratio, measured on the GPU from the raw input, in front of every gain and of the AGC; a field is empty where no level block could be counted\n");
    fprintf(stdout, "\t-m census of transmissions: stderr gets one line per burst of energy in the channel, decoded or not (activity: block <first level block of 512 samples> <duration> ms x<strength over the floor> decoded|crc-failed|missed,\n");
    fprintf(stdout, "\t   with the file name in batch mode and the channel Hz of a list), and at the end of the input a summary per capture and channel (activity: N transmissions, N decoded, N CRC-clean); measured on the GPU from the raw input; stdout does not change\n");
    fprintf(stdout, "\t-x repair time2 telegrams that fail a block CRC: the least reliable chips of a bad block are flipped on the GPU (up to 8 candidates per block, the line code and the CRC decide);\n");
    fprintf(stdout, "\t   a repaired line is printed with CRC flag 1 and ;x<blocks repaired>/<chips flipped> appended (behind -l's and -n's fields, in front of a channel's); with -v stderr gets repair: N subjects, M repaired at the end\n");
    fprintf(stdout, "\t-q append ;<chip rate, chips/s, two decimals>;<jitter ns>;<eye Hz> to every line (behind -l's, -n's and -x's fields, in front of a channel's), e.g. ;99800.14;1367;32214: the transmitter's chip clock,\n");
    fprintf(stdout, "\t   the mean distance of the decision instants from it and the smallest distance of a soft symbol from the decision threshold (0 or less: a chip on the wrong side), measured on the GPU\n");
    fprintf(stdout, "\t   on time2 telegrams decoded whole inside a push; three empty fields on every other line; with -v stderr gets quality: N measured, M with a closed eye at the end\n");
    fprintf(stdout, "\t-y rescue S1 telegrams of the time2 framer that are lost to a Manchester violation: a pair that reads 00 or 11 is decided on the GPU by the larger of its two soft symbols, the block CRCs decide;\n");
    fprintf(stdout, "\t   a rescued line is printed as a clean S1 line with ;y<pairs decided> appended (behind -q's fields, in front of a channel's); with -v stderr gets rescue: N subjects, M rescued at the end\n");
    fprintf(stdout, "\t-w survey the input: a max-hold spectrum of the capture taken on the GPU; at the end of the input stderr gets one line per transmitter found\n");
    fprintf(stdout, "\t   (spectrum: <offset Hz> Hz x<strength> over the floor) and spectrum: -O <offsets>, the -O that decodes them (batch mode: with -S, per file); stdout does not change\n");
    fprintf(stdout, "\t-E seconds the survey of -w and -O auto forgets: it holds the last seconds ... 2 x seconds of the input (epochs of 2^A x 512 samples, the smallest A that\n");
    fprintf(stdout, "\t   lasts that long), so that on a live stream -O auto follows a receiver that drifts and lets go of a transmitter that has gone silent; default: it never forgets\n");
    fprintf(stdout, "\t-B bytes per GPU push (multiple of 4096; default 1048576 for a live stream; per file in batch mode 2097152, 1048576 from 384 files per GPU on)\n");
    fprintf(stdout, "\t-L ms a live stream's bytes wait at most this long for their push to fill (default 50; 0: only full pushes)\n");
    fprintf(stdout, "\t-S batch mode: print samples, seconds and Msamples/s to stderr\n");
    fprintf(stdout, "\t-G HIP device ordinal (default 0); batch mode: 'all' or a list '0,2,5' shards the files, file i on device list[i mod n]\n");
    fprintf(stdout, "\t-M batch mode: print the file -> device map and exit\n");
    fprintf(stdout, "\t-U unique: print a datagram that both the time2 and the run length method decoded only once\n");
    fprintf(stdout, "\t-W like -U, and only datagrams with a correct CRC (what wmbusmeters keeps)\n");
    fprintf(stdout, "\t-A 1|2 atan2_approximation / atan2_approximation2 (atan2.h) instead of cargf in the discriminator\n");
    fprintf(stdout, "\t-F tolerance mode: soft symbols within 2e-6 of the reference's instead of bit-identical (faster; default switches only)\n");
    fprintf(stdout, "\t-P polyphase low-pass (ppf.h) instead of the moving average before decimation (1.6 MS/s, -d 2, no -s)\n");
    fprintf(stdout, "\t-T host:port read the cu8 stream from a TCP server instead of stdin\n");
    fprintf(stdout, "\tFILE... batch mode: decode several cu8 files at once (lines prefixed with the file name)\n");
    fprintf(stdout, "\t-h print this help\n");
}

/* cu8 over TCP: connect and hand back the descriptor (what net_support.h:15-44 offers the reference). */
static int open_tcp(const char *hostport)
{
    char host[256];
    const char *colon = strrchr(hostport, ':');
    if (!colon || colon == hostport || (size_t)(colon - hostport) >= sizeof host) { fprintf(stderr, "rtl_wmbus_hip: -T needs host:port\n"); return -1; }
    memcpy(host, hostport, (size_t)(colon - hostport)); host[colon - hostport] = 0;
    struct addrinfo hints, *res = NULL;
    memset(&hints, 0, sizeof hints);
    hints.ai_family = AF_UNSPEC; hints.ai_socktype = SOCK_STREAM;
    if (getaddrinfo(host, colon + 1, &hints, &res) || !res) { fprintf(stderr, "rtl_wmbus_hip: cannot resolve %s\n", hostport); return -1; }
    int fd = -1;
    for (struct addrinfo *a = res; a; a = a->ai_next) {
        fd = socket(a->ai_family, a->ai_socktype, a->ai_protocol);
        if (fd < 0) continue;
        if (!connect(fd, a->ai_addr, a->ai_addrlen)) break;
        close(fd); fd = -1;
    }
    freeaddrinfo(res);
    if (fd < 0) fprintf(stderr, "rtl_wmbus_hip: cannot connect to %s\n", hostport);
    return fd;
}

/* ---- batch mode ------------------------------------------------------------------------------
 * One wmbus_batch per device (include/wmbus_hip.h): the library splits the device's files over several receiver
 * contexts, drives each on its own thread and overlaps them; this file only supplies the bytes (fread into the page-locked
 * slab the library hands out) and prints the lines. */
/* -m: the census of transmissions (below, in front of batch_lines) */
struct census_line { uint64_t ka; uint32_t stream; uint8_t channel, chain, crc_ok; };
struct census {
    const wmbus_cfg *cfg; char **names;                      /* names: the files of a batch (NULL: a live stream) */
    unsigned fin, n_streams, ch;                             /* channels per capture (1 without a list) */
    uint64_t margin, keep;                                   /* level blocks: 0.15 s; how long a line may wait for its burst */
    wmbus_burst *pend; size_t n_pend, cap_pend;
    struct census_line *lines; size_t n_lines, cap_lines;
    unsigned long long (*sum)[3];                            /* [(stream x ch + channel) x 2 + chain]: transmissions, decoded, CRC-clean */
};

struct batch_job {
    wmbus_cfg cfg; int n; char **names; FILE **f; int *live; int rc;
    unsigned fill_threads;                               /* readers per fill call (a context's files are read side by side) */
    unsigned told;                                       /* warnings already reported for this device */
    int stats, fast_exit, lev_missing;                   /* lev_missing: -l and a push came without its levels (the run fails) */
    wmbus_batch *b;                                      /* -l: the sink asks it for the levels of the lines it is handed */
    wmbus_batch_stats st;
    struct census census;                                /* -m */
    unsigned long long bytes_out, clipped;               /* wmbus_timing.input_bytes_out / input_clipped over the run */
};

static pthread_mutex_t out_lock = PTHREAD_MUTEX_INITIALIZER;      /* one push's lines leave as a unit, whichever device they come from */

/* The reference never stops on an input; neither do we: exhausted chip / burst storage is reported once per device and
 * the stream goes on (wmbus_hip.h, WMBUS_WARN_*).  Callers hold out_lock or are single-threaded. */
static void report_warnings(unsigned warnings, unsigned *told)
{
    if (!(warnings & ~*told)) return;
    if (warnings & ~*told & WMBUS_WARN_CHIPS_DROPPED) fprintf(stderr, "rtl_wmbus_hip: warning: run-length chip storage exhausted (interferer?), some chips dropped; continuing\n");
    if (warnings & ~*told & WMBUS_WARN_BURSTS_DROPPED) fprintf(stderr, "rtl_wmbus_hip: warning: burst storage exhausted, some candidate telegrams dropped; continuing\n");
    *told |= warnings;
}

/* wmbus_batch_io.fill: up to `cap` bytes (whole 4096-byte blocks) of every file of the group; a file that has ended
 * contributes mid-scale bytes (no signal).  Returns the longest contribution; 0 when all have ended.
 * The files of a group are read by several threads side by side: one thread copies page-cache bytes into the page-locked slab
 * at 5-6 GB/s, a context's push of 128 x 2 MiB then takes 43 ms to read against 12 ms on the GPU, and the whole program ran
 * at the readers' 4-8 x 6 GB/s instead of the link's 50 (round 4: 12.9 Gsamples/s over 256 files, 16-17 over 1024). */
struct fill_part { struct batch_job *j; unsigned first, k0, k1; uint8_t *slab; size_t pitch, cap; size_t *got; struct fill_part *next; unsigned *left; };

static void *fill_part_run(void *p)
{
    struct fill_part *q = p;
    for (unsigned k = q->k0; k < q->k1; k++) {
        const unsigned s = q->first + k;
        if (q->j->live[s]) {
            q->got[k] = fread(q->slab + (size_t)k * q->pitch, WMBUS_BLOCK_BYTES, q->cap / WMBUS_BLOCK_BYTES, q->j->f[s]) * WMBUS_BLOCK_BYTES;
            if (q->got[k] < q->cap) q->j->live[s] = 0;
        }
    }
    return NULL;
}

/* The readers are a pool that lives as long as the process (up to 15 threads were created and joined in EVERY fill
 * call, thousands of times per batch, inside the out-of-GPU critical path).  A fill call -- several may run at once, one per context --
 * queues its parts, works on the queue itself and waits for its own parts' count to reach zero. */
static struct { pthread_mutex_t m; pthread_cond_t work, done; struct fill_part *head; unsigned threads; } pool = {PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, NULL, 0};

static struct fill_part *pool_take(void) { struct fill_part *q = pool.head; if (q) pool.head = q->next; return q; }      /* pool.m held */
static void pool_finish(struct fill_part *q)                                                                               /* pool.m held */
{
    if (--*q->left == 0) pthread_cond_broadcast(&pool.done);
}
static void *pool_worker(void *unused)
{
    (void)unused;
    pthread_mutex_lock(&pool.m);
    for (;;) {
        struct fill_part *q = pool_take();
        if (!q) { pthread_cond_wait(&pool.work, &pool.m); continue; }
        pthread_mutex_unlock(&pool.m);
        fill_part_run(q);
        pthread_mutex_lock(&pool.m);
        pool_finish(q);
    }
    return NULL;
}
static void pool_grow(unsigned want)       /* detached workers, started on first use; fewer than asked for is fine (the caller works too) */
{
    pthread_mutex_lock(&pool.m);
    while (pool.threads < want && pool.threads < 64u) {
        pthread_t th;
        if (pthread_create(&th, NULL, pool_worker, NULL)) break;
        pthread_detach(th);
        pool.threads++;
    }
    pthread_mutex_unlock(&pool.m);
}

static size_t batch_fill_padded(void *user, unsigned first, unsigned n, uint8_t *slab, size_t pitch, size_t cap)
{
    struct batch_job *j = user;
    size_t most = 0;
    size_t *got = calloc(n, sizeof *got);
    if (!got) { fprintf(stderr, "rtl_wmbus_hip: out of memory\n"); return 0; }
    unsigned T = j->fill_threads ? j->fill_threads : 1u;
    if (T > 16u) T = 16u;
    if (n < 2u * T) T = 1u;
    struct fill_part part[16];
    unsigned left = T;
    for (unsigned t = 0; t < T; t++) part[t] = (struct fill_part){j, first, (unsigned)((uint64_t)n * t / T), (unsigned)((uint64_t)n * (t + 1) / T), slab, pitch, cap, got, NULL, &left};
    if (T > 1u) {
        pool_grow(8u * (T - 1u));                            /* readers for the contexts that fill at the same time */
        pthread_mutex_lock(&pool.m);
        for (unsigned t = T - 1u; t >= 1u; t--) { part[t].next = pool.head; pool.head = &part[t]; }
        pthread_cond_broadcast(&pool.work);
        pthread_mutex_unlock(&pool.m);
    }
    fill_part_run(&part[0]);
    pthread_mutex_lock(&pool.m);
    pool_finish(&part[0]);
    for (;;) {                                               /* my own parts nobody has taken yet: here; those in other hands: wait */
        struct fill_part *q = NULL, **pp = &pool.head;
        for (; *pp; pp = &(*pp)->next) if ((*pp)->left == &left) { q = *pp; *pp = q->next; break; }
        if (q) { pthread_mutex_unlock(&pool.m); fill_part_run(q); pthread_mutex_lock(&pool.m); pool_finish(q); continue; }
        if (left == 0) break;
        pthread_cond_wait(&pool.done, &pool.m);
    }
    pthread_mutex_unlock(&pool.m);
    for (unsigned k = 0; k < n; k++) if (got[k] > most) most = got[k];
    /* no signal: mid-scale for cu8, zero for the signed formats and for cf32 (0.0f) */
    const int silence = j->cfg.input_format == WMBUS_FMT_CU8 ? 128 : 0;
    for (unsigned k = 0; k < n; k++) if (got[k] < most) memset(slab + (size_t)k * pitch + got[k], silence, most - got[k]);
    free(got);
    return most;
}

/* -l: the line with ";offset_hz;dev_hz" in front of its newline, both fields empty for a level that could not be measured.  -O with a
 * list (chan_hz != NULL): ";<channel Hz>" of the line's channel behind that. */
/* -n: ";signal;noise;x<ratio>" behind -l's fields and in front of the channel's: the power in the telegram's channel, the noise floor in
 * front of it (each empty where no level block could be counted) and the strength the way the spectrum: lines print theirs (empty without
 * either). */
/* -x: the repair records of the lines printed so far (callers hold out_lock or are single-threaded); a subject has a bad block */
static unsigned long long repair_subjects, repair_repaired;
static int line_repaired(const wmbus_repair *rp) { return rp && rp->blocks_bad && rp->blocks_repaired == rp->blocks_bad; }

/* -y: the subjects the decoders took and those rescued, summed over the collects so far (wmbus_rescue_stats), for -v */
static unsigned long long rescue_subjects, rescue_rescued;
static void rescue_count(const wmbus_ctx *ctx)
{
    unsigned s = 0, r = 0;
    if (ctx && wmbus_rescue_stats(ctx, &s, &r) == WMBUS_OK) { rescue_subjects += s; rescue_rescued += r; }
}

/* -q: ";<chip rate, chips/s>;<jitter ns>;<eye Hz>" behind -x's field and in front of the channel's, three empty fields where the line
 * has no quality record (n = 0); the counts of the lines printed so far for -v */
static unsigned long long quality_measured, quality_closed;

/* -y: ";y<pairs decided>" on a rescued line only, behind -q's fields and in front of the channel's */
static void write_line(const char *text, size_t len, const wmbus_level *lev, const wmbus_power *pw, const wmbus_repair *rp, const wmbus_quality *ql, const wmbus_rescue *rs, const int *chan_hz)
{
    if (rs && rs->status != 1u) rs = NULL;                   /* only a rescued line gets the field */
    if (ql && ql->n) { quality_measured++; quality_closed += ql->eye_hz <= 0; }
    if (rp && rp->blocks_bad) { repair_subjects++; repair_repaired += (unsigned)line_repaired(rp); }
    if (!line_repaired(rp)) rp = NULL;                       /* only a repaired line gets the field */
    if (!lev && !pw && !rp && !ql && !rs && !chan_hz) { fwrite(text, 1, len, stdout); return; }
    if (len && text[len - 1] == '\n') len--;
    fwrite(text, 1, len, stdout);
    if (lev && lev->n) fprintf(stdout, ";%d;%u", (int)lev->offset_hz, (unsigned)lev->dev_hz);
    else if (lev) fputs(";;", stdout);
    if (pw) {
        if (pw->n_signal) fprintf(stdout, ";%u", (unsigned)pw->signal); else fputc(';', stdout);
        if (pw->n_noise) fprintf(stdout, ";%u", (unsigned)pw->noise); else fputc(';', stdout);
        if (pw->n_signal && pw->n_noise) fprintf(stdout, ";x%.1f", (double)pw->ratio_q8 / 256.0); else fputc(';', stdout);
    }
    if (rp) fprintf(stdout, ";x%u/%u", (unsigned)rp->blocks_repaired, (unsigned)rp->chips_flipped);
    if (ql && ql->n) fprintf(stdout, ";%u.%02u;%u;%d", (unsigned)(ql->chip_rate_chz / 100u), (unsigned)(ql->chip_rate_chz % 100u), (unsigned)ql->jitter_ns, (int)ql->eye_hz);
    else if (ql) fputs(";;;", stdout);
    if (rs) fprintf(stdout, ";y%u", (unsigned)rs->pairs);
    if (chan_hz) fprintf(stdout, ";%d", *chan_hz);
    fputc('\n', stdout);
}
/* the channel field of a line: only a list of more than one -O entry prints it */
static const int *line_channel_hz(const wmbus_cfg *cfg, const wmbus_line *ln)
{
    return cfg->input_channels > 1u ? &cfg->input_channel_hz[ln->channel] : NULL;
}


/* ---- -m: the census of transmissions (cfg.channel_activity) -------------------------------------------------------------------------
 * Every collect delivers the bursts of energy that closed in it (wmbus_activity) and the lines decoded in it; a line belongs to the burst
 * of its channel that holds its access-code level block (wmbus_activity_match).  A line may come before its burst or after it, so both
 * wait here: a burst is resolved -- decoded, crc-failed or missed -- once the stream has moved 0.15 s, the longest telegram, past its
 * end (wmbus_activity_progress), or at the end of the input.  stderr gets a line per resolved burst and a summary per capture and
 * channel at exit; stdout does not change.  Without -s both chains listen on the same channel and see the same bursts: the T1/C1 row's
 * are counted, lines of either chain match them.  Callers hold out_lock or are single-threaded. */
static int census_open(struct census *cs, const wmbus_cfg *cfg, unsigned n_streams, char **names)
{
    memset(cs, 0, sizeof *cs);
    cs->cfg = cfg; cs->names = names; cs->n_streams = n_streams;
    cs->fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
    cs->ch = cfg->input_channels > 1u ? cfg->input_channels : 1u;
    cs->margin = (3ull * cs->fin + 10239u) / 10240u;         /* ceil(0.15 Fin / 512) */
    cs->keep = cs->margin + 66u * 64u;                       /* the longest run the floor allows (H + 2 <= 65 epochs), and its epoch's end */
    cs->sum = calloc((size_t)n_streams * cs->ch * 2u, sizeof *cs->sum);
    return cs->sum ? 0 : -1;
}

static void census_print_row(const struct census *cs, unsigned stream, unsigned channel, unsigned chain)
{
    if (cs->names) fprintf(stderr, "%s: ", cs->names[stream]);
    fputs("activity", stderr);
    if (cs->ch > 1u && cs->cfg->simultaneous) fprintf(stderr, "[%d %s]", cs->cfg->input_channel_hz[channel], chain ? "S1" : "T1/C1");
    else if (cs->ch > 1u) fprintf(stderr, "[%d]", cs->cfg->input_channel_hz[channel]);
    else if (cs->cfg->simultaneous) fprintf(stderr, "[%s]", chain ? "S1" : "T1/C1");
    fputs(": ", stderr);
}

/* first: the context's first stream (a batch); progress: the context's level blocks so far; all: the input has ended, resolve everything
 * of streams [first, first + n) */
static void census_resolve(struct census *cs, unsigned first, unsigned n, uint64_t progress, int all)
{
    size_t kept = 0;
    for (size_t i = 0; i < cs->n_pend; i++) {
        const wmbus_burst *b = &cs->pend[i];
        if (b->stream < first || b->stream >= first + n) { cs->pend[kept++] = *b; continue; }
        if (!all && progress < b->first_block + b->blocks + cs->margin) { cs->pend[kept++] = *b; continue; }
        int matched = 0, clean = 0;
        for (size_t k = 0; k < cs->n_lines; k++) {
            const struct census_line *l = &cs->lines[k];
            if (wmbus_activity_match(b, 1, l->stream, l->channel, cs->cfg->simultaneous ? l->chain : b->chain, l->ka) == 0) { matched = 1; clean |= l->crc_ok; }
        }
        unsigned long long *sum = cs->sum[((size_t)b->stream * cs->ch + b->channel) * 2u + b->chain];
        sum[0]++; sum[1] += (unsigned)matched; sum[2] += (unsigned)clean;
        census_print_row(cs, b->stream, b->channel, b->chain);
        fprintf(stderr, "block %llu %.1f ms x%.1f %s\n", (unsigned long long)b->first_block, (double)b->blocks * 512e3 / (double)cs->fin,
                (double)b->mean / (double)(b->floor ? b->floor : 1u), clean ? "decoded" : matched ? "crc-failed" : "missed");
    }
    cs->n_pend = kept;
    kept = 0;                                                /* a line too old for any burst still to come leaves */
    for (size_t k = 0; k < cs->n_lines; k++) {
        const struct census_line *l = &cs->lines[k];
        const int mine = l->stream >= first && l->stream < first + n;
        if (mine && (all || l->ka + cs->keep < progress)) continue;
        cs->lines[kept++] = *l;
    }
    cs->n_lines = kept;
}

/* one collect of one context: its lines (stream already counted over the whole batch), their levels, its bursts (stream counted from `first`) */
static int census_push(struct census *cs, unsigned first, unsigned n, const wmbus_line *ln, const wmbus_level *lev, size_t nl, const wmbus_burst *bu, size_t nb, uint64_t progress)
{
    if (cs->n_lines + nl > cs->cap_lines) {
        void *p = realloc(cs->lines, (cs->n_lines + nl + 64u) * sizeof *cs->lines);
        if (!p) return -1;
        cs->lines = p; cs->cap_lines = cs->n_lines + nl + 64u;
    }
    if (cs->n_pend + nb > cs->cap_pend) {
        void *p = realloc(cs->pend, (cs->n_pend + nb + 64u) * sizeof *cs->pend);
        if (!p) return -1;
        cs->pend = p; cs->cap_pend = cs->n_pend + nb + 64u;
    }
    for (size_t i = 0; i < nl; i++) {
        uint64_t ka = 0;
        if (wmbus_line_power_block(cs->cfg->decimation, cs->cfg->input_rate_hz, lev[i].sync_sample, &ka)) continue;
        cs->lines[cs->n_lines++] = (struct census_line){ka, ln[i].stream, ln[i].channel, ln[i].chain, ln[i].crc_ok};
    }
    for (size_t i = 0; i < nb; i++) {
        if (!cs->cfg->simultaneous && bu[i].chain != WMBUS_CHAIN_T1C1) continue;
        cs->pend[cs->n_pend] = bu[i];
        cs->pend[cs->n_pend++].stream += first;
    }
    census_resolve(cs, first, n, progress, 0);
    return 0;
}

static void census_close(struct census *cs)
{
    for (unsigned s = 0; s < cs->n_streams; s++)
        for (unsigned c = 0; c < cs->ch; c++)
            for (unsigned chain = 0; chain < (cs->cfg->simultaneous ? 2u : 1u); chain++) {
                const unsigned long long *sum = cs->sum[((size_t)s * cs->ch + c) * 2u + chain];
                census_print_row(cs, s, c, chain);
                fprintf(stderr, "%llu transmissions, %llu decoded, %llu CRC-clean\n", sum[0], sum[1], sum[2]);
            }
    free(cs->pend); free(cs->lines); free(cs->sum);
    memset(cs, 0, sizeof *cs);
}

static void batch_lines(void *user, unsigned first, unsigned n, const wmbus_line *ln, size_t nl, const char *text, const wmbus_timing *t)
{
    struct batch_job *j = user;
    const wmbus_level *lev = NULL;
    const wmbus_power *pw = NULL;
    const wmbus_repair *rp = NULL;
    const wmbus_quality *ql = NULL;
    const wmbus_rescue *rs = NULL;
    pthread_mutex_lock(&out_lock);
    if ((j->cfg.line_levels && wmbus_batch_line_levels(j->b, first, &lev) != nl) || (j->cfg.line_power && wmbus_batch_line_power(j->b, first, &pw) != nl) ||
        (j->cfg.crc_repair && wmbus_batch_line_repairs(j->b, first, &rp) != nl) || (j->cfg.line_quality && wmbus_batch_line_quality(j->b, first, &ql) != nl) ||
        (j->cfg.s1_rescue && wmbus_batch_line_rescues(j->b, first, &rs) != nl)) {      /* cannot happen: a level per line.  Never print lines with fewer fields than -l promises */
        fprintf(stderr, "rtl_wmbus_hip: internal error: the levels of %zu lines are missing; the lines are not printed\n", nl);
        j->lev_missing = 1;
        pthread_mutex_unlock(&out_lock);
        return;
    }
    report_warnings(t->warnings, &j->told);
    j->bytes_out += t->input_bytes_out; j->clipped += t->input_clipped;
    for (size_t i = 0; i < nl; i++) {
        fputs(j->names[ln[i].stream], stdout); fputs(": ", stdout);
        write_line(text + ln[i].text_off, ln[i].text_len, j->cfg.line_levels && lev ? lev + i : NULL, j->cfg.line_power && pw ? pw + i : NULL, rp ? rp + i : NULL, ql ? ql + i : NULL, rs ? rs + i : NULL, line_channel_hz(&j->cfg, ln + i));
    }
    if (nl) fflush(stdout);
    if (j->cfg.s1_rescue)                                    /* -y: this collect's counts */
        for (unsigned i = 0; i < wmbus_batch_contexts(j->b); i++) {
            unsigned f = 0, m = 0;
            wmbus_ctx *ctx = wmbus_batch_context(j->b, i, &f, &m);
            if (ctx && f == first) rescue_count(ctx);
        }
    if (j->cfg.channel_activity) {                           /* -m: this collect's bursts and lines into the census */
        const wmbus_burst *bu = NULL;
        const wmbus_level *lv = NULL;
        const size_t nb = wmbus_batch_activity(j->b, first, &bu);
        uint64_t progress = 0;
        for (unsigned i = 0; i < wmbus_batch_contexts(j->b); i++) {
            unsigned f = 0, m = 0;
            wmbus_ctx *ctx = wmbus_batch_context(j->b, i, &f, &m);
            if (ctx && f == first) progress = wmbus_activity_progress(ctx);
        }
        if (wmbus_batch_line_levels(j->b, first, &lv) != nl || census_push(&j->census, first, n, ln, lv, nl, bu, nb, progress)) j->lev_missing = 1;
    }
    pthread_mutex_unlock(&out_lock);
}

/* -w: the survey of one capture of a context at the end of its input, to stderr: a line per hit and the -O that decodes them */
static void print_spectrum(wmbus_ctx *ctx, unsigned stream, const wmbus_cfg *cfg, const char *name)
{
    uint64_t sum[512];
    uint32_t peak[512];
    uint64_t blocks = 0;
    wmbus_channel_hit hit[WMBUS_MAX_CHANNELS];
    const char *sep = name ? ": " : "";
    if (!name) name = "";
    if (wmbus_read_spectrum(ctx, stream, sum, peak, &blocks, 0) < 0) { fprintf(stderr, "rtl_wmbus_hip: %s%s%s\n", name, sep, wmbus_last_error(ctx)); return; }
    const unsigned fin = cfg->input_rate_hz ? cfg->input_rate_hz : cfg->decimation * 800000u;
    const int n = blocks ? wmbus_spectrum_channels(fin, sum, peak, blocks, 0, 0, 0, hit, WMBUS_MAX_CHANNELS) : 0;
    if (n <= 0) { fprintf(stderr, "%s%sspectrum: nothing above the floor\n", name, sep); return; }
    for (int k = 0; k < n; k++) fprintf(stderr, "%s%sspectrum: %d Hz x%.1f over the floor\n", name, sep, (int)hit[k].offset_hz, (double)hit[k].ratio_q8 / 256.0);
    fprintf(stderr, "%s%sspectrum: -O ", name, sep);
    for (int k = 0; k < n; k++) fprintf(stderr, "%s%d", k ? "," : "", (int)hit[k].offset_hz);
    fputc('\n', stderr);
}

static void print_afc(wmbus_ctx *ctx, unsigned stream, const char *name, unsigned *seen, const int *chan_hz);
static int any_channel_afc(const wmbus_cfg *cfg);

static int run_batch(struct batch_job *j)
{
    int rc = EXIT_FAILURE;
    wmbus_batch *b = NULL;
    j->f = calloc((size_t)j->n, sizeof *j->f); j->live = calloc((size_t)j->n, sizeof *j->live);
    if (!j->f || !j->live) goto out;
    for (int s = 0; s < j->n; s++) {
        j->f[s] = fopen(j->names[s], "rb");
        if (!j->f[s]) { fprintf(stderr, "rtl_wmbus_hip: cannot open %s\n", j->names[s]); goto out; }
        j->live[s] = 1;
    }
    j->cfg.n_streams = (unsigned)j->n;
    j->cfg.input_windows = 2;                                /* the next push crosses PCIe while the previous one is in flight */
    struct timespec t_open0, t_open1;
    clock_gettime(CLOCK_MONOTONIC, &t_open0);
    if (wmbus_batch_open(&j->cfg, 0, &b)) {
        fprintf(stderr, "rtl_wmbus_hip: cannot open GPU back end: %s\n", b ? wmbus_batch_last_error(b) : "out of memory");
        goto out;
    }
    clock_gettime(CLOCK_MONOTONIC, &t_open1);
    j->b = b;
    if (j->cfg.channel_activity && census_open(&j->census, &j->cfg, (unsigned)j->n, j->names)) { fprintf(stderr, "rtl_wmbus_hip: out of memory\n"); goto out; }
    if (j->stats) fprintf(stderr, "rtl_wmbus_hip: device %d: contexts open after %.3f s\n", j->cfg.device, (double)(t_open1.tv_sec - t_open0.tv_sec) + (t_open1.tv_nsec - t_open0.tv_nsec) * 1e-9);
    wmbus_batch_io io;
    memset(&io, 0, sizeof io);
    io.fill = batch_fill_padded; io.lines = batch_lines; io.user = j;
    if (wmbus_batch_run(b, &io, &j->st)) { fprintf(stderr, "rtl_wmbus_hip: %s\n", wmbus_batch_last_error(b)); goto out; }
    if (j->cfg.channel_activity) {                           /* -m: what is still open is resolved by the end of the input, then every file's summary */
        pthread_mutex_lock(&out_lock);
        census_resolve(&j->census, 0, (unsigned)j->n, 0, 1);
        census_close(&j->census);
        pthread_mutex_unlock(&out_lock);
    }
    if (j->stats) {
        unsigned lanes = 0;
        unsigned long long paired = 0, single = 0;
        wmbus_batch_lane_stats(b, &lanes, &paired, &single);
        fprintf(stderr, "rtl_wmbus_hip: device %d: %d files, %u contexts, %llu samples, %llu lines, %u pushes in %.3f s = %.1f Msamples/s; %u lanes, %llu paired and %llu single kernel launches\n",
                j->cfg.device, j->n, wmbus_batch_contexts(b), (unsigned long long)j->st.samples, (unsigned long long)j->st.lines, j->st.pushes, j->st.seconds,
                j->st.seconds > 0 ? (double)j->st.samples / j->st.seconds / 1e6 : 0.0, lanes, paired, single);
    }
    if (j->stats && j->bytes_out)                            /* a converting path is active: what the gain did */
        fprintf(stderr, "rtl_wmbus_hip: device %d: input conversion: %llu of %llu bytes clipped (%.4f %%)\n", j->cfg.device, j->clipped, j->bytes_out,
                100.0 * (double)j->clipped / (double)j->bytes_out);
    if (j->stats && j->cfg.input_spectrum)                   /* -w: every file's survey, read from the context that served it */
        for (unsigned i = 0; i < wmbus_batch_contexts(b); i++) {
            unsigned first = 0, n = 0;
            wmbus_ctx *ctx = wmbus_batch_context(b, i, &first, &n);
            pthread_mutex_lock(&out_lock);                   /* a file's lines leave as a unit, whichever device they come from */
            for (unsigned s = 0; ctx && s < n; s++) print_spectrum(ctx, s, &j->cfg, j->names[first + s]);
            pthread_mutex_unlock(&out_lock);
        }
    if (j->cfg.input_afc && j->cfg.show_algorithm)           /* -O auto -v: the lock every file ended with */
        for (unsigned i = 0; i < wmbus_batch_contexts(b); i++) {
            unsigned first = 0, n = 0;
            wmbus_ctx *ctx = wmbus_batch_context(b, i, &first, &n);
            pthread_mutex_lock(&out_lock);
            for (unsigned s = 0; ctx && s < n; s++) print_afc(ctx, s, j->names[first + s], NULL, NULL);
            pthread_mutex_unlock(&out_lock);
        }
    if (any_channel_afc(&j->cfg) && j->cfg.show_algorithm)   /* a list with auto: entries and -v: every file's final lock per following channel */
        for (unsigned i = 0; i < wmbus_batch_contexts(b); i++) {
            unsigned first = 0, n = 0;
            wmbus_ctx *ctx = wmbus_batch_context(b, i, &first, &n);
            pthread_mutex_lock(&out_lock);
            for (unsigned s = 0; ctx && s < n; s++)
                for (unsigned ch = 0; ch < j->cfg.input_channels; ch++)
                    if (j->cfg.input_channel_afc_hz[ch]) print_afc(ctx, s * j->cfg.input_channels + ch, j->names[first + s], NULL, &j->cfg.input_channel_hz[ch]);
            pthread_mutex_unlock(&out_lock);
        }
    rc = j->lev_missing ? EXIT_FAILURE : EXIT_SUCCESS;
out:
    if (!j->fast_exit || rc != EXIT_SUCCESS) wmbus_batch_close(b);      /* every exit path closes what it opened, unless the process is about to end anyway */
    for (int s = 0; j->f && s < j->n; s++) if (j->f[s]) fclose(j->f[s]);
    free(j->f); free(j->live);
    return rc;
}

/* File i of a batch -> position in the device list (stream s -> GPU s mod n).  The only place
 * the map is defined; -M prints it, tests/test_multi_gloo.py holds it against rtl-wmbus_amd/shard.py. */
static int shard_slot(int file_index, int n_devices) { return file_index % n_devices; }

/* ---- batch mode over several GPUs: one batch per device, each on its own thread ---------- */
static void *shard_thread(void *p) { struct batch_job *j = p; j->rc = j->n ? run_batch(j) : EXIT_SUCCESS; return NULL; }

static int run_sharded(wmbus_cfg cfg, int n, char **names, const int *devs, int n_devs, int map_only, int stats)
{
    struct batch_job *jobs = calloc((size_t)n_devs, sizeof *jobs);
    pthread_t *th = calloc((size_t)n_devs, sizeof *th);
    /* host decoder threads per context: devices x contexts (8 per batch) x threads within the host's hardware threads */
    long cpus = sysconf(_SC_NPROCESSORS_ONLN);
    if (cpus < 1) cpus = 16;
    unsigned per_ctx = (unsigned)(cpus / (8L * n_devs));
    if (per_ctx < 1) per_ctx = 1;
    if (per_ctx > 16) per_ctx = 16;
    if (cfg.host_threads == 0 && n_devs > 1) cfg.host_threads = per_ctx;
    /* file readers per context: the host's threads over the devices' contexts, half of them (the decoder threads want the rest) */
    unsigned readers = (unsigned)(cpus / (16L * n_devs));
    if (readers < 1) readers = 1;
    if (readers > 8) readers = 8;
    for (int k = 0; k < n_devs; k++) jobs[k].fill_threads = readers;
    for (int k = 0; k < n_devs; k++) { jobs[k].cfg = cfg; jobs[k].cfg.device = devs[k]; jobs[k].names = calloc((size_t)n, sizeof(char *)); jobs[k].stats = stats; jobs[k].fast_exit = !getenv("WMBUS_SLOW_EXIT"); }
    for (int i = 0; i < n; i++) {
        const int k = shard_slot(i, n_devs);
        jobs[k].names[jobs[k].n++] = names[i];
        if (map_only) fprintf(stdout, "%s -> device %d\n", names[i], devs[k]);
    }
    int rc = EXIT_SUCCESS;
    if (!map_only) {
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int k = 1; k < n_devs; k++) pthread_create(&th[k], NULL, shard_thread, &jobs[k]);
        shard_thread(&jobs[0]);
        if (jobs[0].rc) rc = jobs[0].rc;
        for (int k = 1; k < n_devs; k++) { pthread_join(th[k], NULL); if (jobs[k].rc) rc = jobs[k].rc; }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (stats) {
            unsigned long long samples = 0; double run_s = 0;
            for (int k = 0; k < n_devs; k++) { samples += jobs[k].st.samples; if (jobs[k].st.seconds > run_s) run_s = jobs[k].st.seconds; }
            const double wall = (double)(t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) * 1e-9;
            fprintf(stderr, "rtl_wmbus_hip: total: %d files on %d device(s), %llu samples; decode %.3f s = %.1f Msamples/s; with set-up (contexts, page-locked staging) %.3f s = %.1f Msamples/s\n",
                    n, n_devs, samples, run_s, run_s > 0 ? samples / run_s / 1e6 : 0.0, wall, wall > 0 ? samples / wall / 1e6 : 0.0);
        }
    }
    for (int k = 0; k < n_devs; k++) free(jobs[k].names);
    free(jobs); free(th);
    return rc;
}

/* The last thing a batch run does: every line is out, and the process ends HERE.  An orderly teardown (unpinning 16 GB of
 * staging, freeing 44 GB of HBM, the HIP runtime's own exit handlers) took 1.5 s of a 1024-file job's 5 s; the driver
 * reclaims all of it when the process is gone.  Library callers that live on use wmbus_batch_close. */
static void finish(int rc)
{
    fflush(stdout); fflush(stderr);
    if (getenv("WMBUS_SLOW_EXIT")) exit(rc);             /* tests / leak checkers: every batch has been closed (run_batch), the runtime's exit handlers run */
    _exit(rc);
}

/* -R: "2048000" | "2.048M" | "2048k" -> Hz; 0 if it is not a rate */
static unsigned parse_rate(const char *arg)
{
    char *end;
    const double v = strtod(arg, &end);
    double mul = 1.;
    if (end == arg || !(v > 0.)) return 0;
    if (*end == 'M' || *end == 'm') { mul = 1e6; end++; }
    else if (*end == 'k' || *end == 'K') { mul = 1e3; end++; }
    if (*end) return 0;
    const double hz = v * mul + 0.5;
    if (hz < 1. || hz > 4294967295.) return 0;
    const unsigned r = (unsigned)hz;
    return (double)r - v * mul > 1e-3 || v * mul - (double)r > 1e-3 ? 0 : r;      /* a whole number of Hz */
}

/* -O: a signed rate, "-250k" | "1e5" | "0.25M" -> Hz; 0 is a valid answer, so *ok says whether it is one */
static int parse_shift(const char *arg, int *ok)
{
    const int neg = arg[0] == '-';
    *ok = 0;
    if (arg[0] == '-' || arg[0] == '+') arg++;
    if (arg[0] == '-' || arg[0] == '+') return 0;
    char *end;
    const double v = strtod(arg, &end);
    if (end != arg && v == 0. && (!*end || ((*end == 'k' || *end == 'K' || *end == 'M' || *end == 'm') && !end[1]))) { *ok = 1; return 0; }
    const unsigned hz = parse_rate(arg);
    if (!hz || hz > 2147483647u) return 0;
    *ok = 1;
    return neg ? -(int)hz : (int)hz;
}

/* -I: the format's WMBUS_FMT_*, or -1 */
static int parse_format(const char *arg)
{
    static const char *const names[] = {"cu8", "cs8", "cs16", "cf32"};      /* index = WMBUS_FMT_* */
    for (int k = 0; k < 4; k++) if (!strcmp(arg, names[k])) return k;
    return -1;
}

/* -g: decimal dB (may be negative) -> linear gain in Q8, clamp(rint(256 * 10^(dB / 20)), 1, 65535); 0 if it is not a number */
static unsigned parse_gain_db(const char *arg)
{
    char *end;
    const double db = strtod(arg, &end);
    if (end == arg || *end || !(db == db) || db > 1000. || db < -1000.) return 0;
    const double q = rint(256. * pow(10., db / 20.));
    return q < 1. ? 1u : q > 65535. ? 65535u : (unsigned)q;
}

/* -G: "3" | "all" | "0,2,5" -> device list; returns the count or -1 */
static int parse_devices(const char *arg, int *devs, int cap)
{
    if (!strcmp(arg, "all")) {
        int n = wmbus_device_count();
        if (n > cap) n = cap;
        for (int k = 0; k < n; k++) devs[k] = k;
        return n;                                            /* 0: no HIP device */
    }
    int n = 0;
    const char *p = arg;
    while (*p) {
        char *end;
        const long v = strtol(p, &end, 10);
        if (end == p || v < 0 || n == cap) return -1;
        devs[n++] = (int)v;
        if (*end == ',') end++; else if (*end) return -1;
        p = end;
    }
    return n ? n : -1;
}

/* ---- live stream (stdin / TCP): wm_reader.c stages the bytes, this is where a push leaves -------- */
struct live { wmbus_ctx *ctx; unsigned told; int levels; const wmbus_cfg *cfg; unsigned afc_changes; unsigned afc_ch_changes[WMBUS_MAX_CHANNELS]; struct census census; };

/* a list with auto: entries (cfg.input_channel_afc_hz): is any channel following its transmitter? */
static int any_channel_afc(const wmbus_cfg *cfg)
{
    for (unsigned ch = 0; ch < cfg->input_channels && ch < WMBUS_MAX_CHANNELS; ch++) if (cfg->input_channel_afc_hz[ch]) return 1;
    return 0;
}

/* -O auto with -v: the lock of one capture to stderr where it has changed since `*seen` changes (NULL: print it if there is one).
 * chan_hz: NULL, or the channel of a list whose lock `stream` (capture x channels + channel) is: the line says afc[<channel Hz>]: */
static void print_afc(wmbus_ctx *ctx, unsigned stream, const char *name, unsigned *seen, const int *chan_hz)
{
    wmbus_afc a;
    const char *sep = name ? ": " : "";
    if (!name) name = "";
    if (wmbus_read_input_afc(ctx, stream, &a) < 0) { fprintf(stderr, "rtl_wmbus_hip: %s%s%s\n", name, sep, wmbus_last_error(ctx)); return; }
    if (seen ? a.changes == *seen : !a.locked) return;
    if (seen) *seen = a.changes;
    if (chan_hz) fprintf(stderr, "%s%safc[%d]: %d Hz x%.1f over the floor\n", name, sep, *chan_hz, (int)a.shift_hz, (double)a.ratio_q8 / 256.0);
    else fprintf(stderr, "%s%safc: %d Hz x%.1f over the floor\n", name, sep, (int)a.shift_hz, (double)a.ratio_q8 / 256.0);
}

static int live_push(void *user, const unsigned char *buf, size_t n)
{
    struct live *lv = user;
    int rc = wmbus_stage(lv->ctx, 0, buf, n);
    if (!rc) rc = wmbus_process(lv->ctx, n);
    if (!rc) rc = wmbus_collect(lv->ctx);
    if (rc) { fprintf(stderr, "rtl_wmbus_hip: %s\n", wmbus_last_error(lv->ctx)); return rc; }
    wmbus_timing t;
    if (!wmbus_get_timing(lv->ctx, &t)) report_warnings(t.warnings, &lv->told);
    if (lv->cfg->input_afc && lv->cfg->show_algorithm) print_afc(lv->ctx, 0, NULL, &lv->afc_changes, NULL);
    if (lv->cfg->show_algorithm)                             /* a list with auto: entries: every following channel's lock */
        for (unsigned ch = 0; ch < lv->cfg->input_channels; ch++)
            if (lv->cfg->input_channel_afc_hz[ch]) print_afc(lv->ctx, ch, NULL, &lv->afc_ch_changes[ch], &lv->cfg->input_channel_hz[ch]);
    if (lv->cfg->channel_activity) {                         /* -m */
        const wmbus_line *ln; const wmbus_level *lev = NULL; const wmbus_burst *bu = NULL;
        const size_t nl = wmbus_lines(lv->ctx, &ln), nb = wmbus_activity(lv->ctx, &bu);
        if (wmbus_line_levels(lv->ctx, &lev) != nl || census_push(&lv->census, 0, 1, ln, lev, nl, bu, nb, wmbus_activity_progress(lv->ctx))) {
            fprintf(stderr, "rtl_wmbus_hip: internal error: the levels of %zu lines are missing\n", nl);
            return -1;
        }
    }
    size_t len = 0;
    const char *text = wmbus_lines_text(lv->ctx, &len);
    if (lv->cfg->s1_rescue) rescue_count(lv->ctx);
    if (len && (lv->levels || lv->cfg->line_power || lv->cfg->crc_repair || lv->cfg->line_quality || lv->cfg->s1_rescue || lv->cfg->input_channels > 1u)) {
        const wmbus_line *ln; const wmbus_level *lev = NULL;
        const wmbus_power *pw = NULL;
        const wmbus_repair *rp = NULL;
        const wmbus_quality *ql = NULL;
        const wmbus_rescue *rs = NULL;
        const size_t nl = wmbus_lines(lv->ctx, &ln);
        if ((lv->levels && wmbus_line_levels(lv->ctx, &lev) != nl) || (lv->cfg->line_power && wmbus_line_power(lv->ctx, &pw) != nl) ||
            (lv->cfg->crc_repair && wmbus_line_repairs(lv->ctx, &rp) != nl) || (lv->cfg->line_quality && wmbus_line_quality(lv->ctx, &ql) != nl) ||
            (lv->cfg->s1_rescue && wmbus_line_rescues(lv->ctx, &rs) != nl)) {      /* cannot happen: a level per line.  Never print lines with fewer fields than -l promises */
            fprintf(stderr, "rtl_wmbus_hip: internal error: the levels of %zu lines are missing\n", nl);
            return -1;
        }
        for (size_t i = 0; i < nl; i++) write_line(text + ln[i].text_off, ln[i].text_len, lv->levels && lev ? lev + i : NULL, pw ? pw + i : NULL, rp ? rp + i : NULL, ql ? ql + i : NULL, rs ? rs + i : NULL, line_channel_hz(lv->cfg, ln + i));
        fflush(stdout);
    } else if (len) { fwrite(text, 1, len, stdout); fflush(stdout); }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 1 && isatty(0)) { print_usage(argv[0]); return 0; }
    wmbus_runtime_init();                                    /* before the first HIP call, before any thread exists */

    wmbus_cfg cfg;
    wmbus_default_cfg(&cfg);
    cfg.max_push_bytes = 0;                                  /* 0: the mode's default, see below */
    int check_flow = 0, opt, map_only = 0, devs[64], n_devs = 0, stats = 0, gain_given = 0;
    double age_seconds = 0.0;                                /* -E */
    unsigned max_latency_ms = 50;
    const char *tcp = NULL;
    while ((opt = getopt(argc, argv, "ofad:p:r:vVst:B:G:PT:A:MUWL:SFR:I:g:O:C:lwE:nmxqy")) != -1) {
        switch (opt) {
        case 'o': cfg.remove_dc = 1; break;
        case 'f': check_flow = 1; break;
        case 'a': cfg.accurate_atan = 0; break;
        case 'p':
            if (!strcmp(optarg, "T") || !strcmp(optarg, "t")) cfg.t1c1_enabled = 0;
            else if (!strcmp(optarg, "S") || !strcmp(optarg, "s")) cfg.s1_enabled = 0;
            else { print_usage(argv[0]); return EXIT_FAILURE; }
            break;
        case 'r': if (strcmp(optarg, "0")) { print_usage(argv[0]); return EXIT_FAILURE; } cfg.rla_enabled = 0; break;
        case 't': if (strcmp(optarg, "0")) { print_usage(argv[0]); return EXIT_FAILURE; } cfg.time2_enabled = 0; break;
        case 'd': cfg.decimation = (unsigned)strtoul(optarg, NULL, 10); break;
        case 's': cfg.simultaneous = 1; break;
        case 'v': cfg.show_algorithm = 1; break;
        case 'V': fprintf(stdout, "rtl_wmbus: " VERSION "\n"); fprintf(stdout, COMMIT "\n"); return EXIT_SUCCESS;    /* two lines: version, commit (rtl_wmbus.c:886-890) */
        case 'B': cfg.max_push_bytes = (size_t)strtoull(optarg, NULL, 10) / WMBUS_BLOCK_BYTES * WMBUS_BLOCK_BYTES; break;
        case 'G':
            n_devs = parse_devices(optarg, devs, 64);
            if (n_devs < 0) { print_usage(argv[0]); return EXIT_FAILURE; }
            if (n_devs == 0) { fprintf(stderr, "rtl_wmbus_hip: -G all: no HIP device (this program has no CPU fallback)\n"); return EXIT_FAILURE; }
            cfg.device = devs[0];
            break;
        case 'M': map_only = 1; break;
        case 'U': cfg.dedup_twins = 1; break;
        case 'W': cfg.dedup_twins = 1; cfg.only_crc_ok = 1; break;
        case 'P': cfg.prefilter = WMBUS_PREFILTER_POLYPHASE; break;
        case 'A': cfg.atan_mode = atoi(optarg); break;
        case 'T': tcp = optarg; break;
        case 'L': max_latency_ms = (unsigned)strtoul(optarg, NULL, 10); break;
        case 'S': stats = 1; break;
        case 'l': cfg.line_levels = 1; break;
        case 'n': cfg.line_power = 1; break;
        case 'm': cfg.channel_activity = 1; break;
        case 'x': cfg.crc_repair = 1; break;
        case 'q': cfg.line_quality = 1; break;
        case 'y': cfg.s1_rescue = 1; break;
        case 'w': cfg.input_spectrum = 1; break;
        case 'E': {
            char *end;
            age_seconds = strtod(optarg, &end);
            if (end == optarg || *end || !(age_seconds > 0.0) || age_seconds > 1e9) { print_usage(argv[0]); return EXIT_FAILURE; }
            break;
        }
        case 'F': cfg.tolerance_mode = 1; break;
        case 'R':
            cfg.input_rate_hz = parse_rate(optarg);
            if (!cfg.input_rate_hz) { print_usage(argv[0]); return EXIT_FAILURE; }
            break;
        case 'I': {
            const int f = parse_format(optarg);
            if (f < 0) { print_usage(argv[0]); return EXIT_FAILURE; }
            cfg.input_format = (unsigned)f;
            break;
        }
        case 'O': {                                          /* one offset, or a comma-separated list of channels, each spelled alike */
            char item[64];
            unsigned n = 0;
            memset(cfg.input_channel_afc_hz, 0, sizeof cfg.input_channel_afc_hz);
            if (!strncmp(optarg, "auto", 4) && !strchr(optarg, ',')) {       /* auto | auto:HZ -- AFC around the nominal, per capture */
                int ok = 1;
                const int nominal = optarg[4] == ':' ? parse_shift(optarg + 5, &ok) : 0;
                if (!ok || (optarg[4] && optarg[4] != ':')) { print_usage(argv[0]); return EXIT_FAILURE; }
                cfg.input_afc = 1; cfg.input_shift_hz = nominal; cfg.input_channels = 0;
                break;
            }
            cfg.input_afc = 0;
            for (const char *p = optarg;; ) {
                const char *comma = strchr(p, ',');
                const size_t len = comma ? (size_t)(comma - p) : strlen(p);
                int ok = 0;
                if (len == 0 || len >= sizeof item || n == WMBUS_MAX_CHANNELS) { print_usage(argv[0]); return EXIT_FAILURE; }
                memcpy(item, p, len); item[len] = 0;
                /* an entry of a list: HZ (fixed) or auto:HZ (that channel follows its transmitter within the default range); a bare auto
                 * inside a list, auto: and auto:x are bad options */
                const int follows = !strncmp(item, "auto", 4);
                if (follows && item[4] != ':') { print_usage(argv[0]); return EXIT_FAILURE; }
                cfg.input_channel_afc_hz[n] = follows ? 64000u : 0u;
                cfg.input_channel_hz[n++] = parse_shift(follows ? item + 5 : item, &ok);
                if (!ok) { print_usage(argv[0]); return EXIT_FAILURE; }
                if (!comma) break;
                p = comma + 1;
            }
            /* one entry is the shift it always was; more are the channels of a wideband capture */
            cfg.input_shift_hz = n == 1u ? cfg.input_channel_hz[0] : 0;
            cfg.input_channels = n == 1u ? 0u : n;
            if (n == 1u) { cfg.input_channel_hz[0] = 0; cfg.input_channel_afc_hz[0] = 0; }
            break;
        }
        case 'C': {
            char *end;
            const long r = strtol(optarg, &end, 10);
            if (end == optarg || *end || r < 1 || r > 12) { print_usage(argv[0]); return EXIT_FAILURE; }
            cfg.input_dc = (unsigned)r;
            break;
        }
        case 'g':
            if (!strcmp(optarg, "auto")) { cfg.input_agc = 1; break; }
            cfg.input_gain_q8 = parse_gain_db(optarg);
            if (!cfg.input_gain_q8) { print_usage(argv[0]); return EXIT_FAILURE; }
            gain_given = 1;
            break;
        default: print_usage(argv[0]); return EXIT_FAILURE;
        }
    }
    if (cfg.input_agc && gain_given) { print_usage(argv[0]); return EXIT_FAILURE; }      /* -g auto takes the place of a gain in dB */
    if (age_seconds > 0.0) {                                 /* -E: the smallest A whose epoch of 2^A x 512 input samples lasts that long */
        if (!cfg.input_spectrum && !cfg.input_afc && !any_channel_afc(&cfg)) { print_usage(argv[0]); return EXIT_FAILURE; }      /* nothing would be surveyed */
        const double want = age_seconds * (double)(cfg.input_rate_hz ? cfg.input_rate_hz : (cfg.decimation ? cfg.decimation : 1u) * 800000u);
        unsigned a = 1u;
        while (a < 31u && (double)(1ull << a) * 512.0 < want) a++;
        cfg.input_spectrum_age = a;
    }
    if (getenv("WMBUS_FIXED_TS")) cfg.fixed_timestamp = 1;
    /* -d is taken unchecked like the reference takes it (rtl_wmbus.c:950).  There `-d 0` keeps every sample, exactly like
     * `-d 1` (the counter test at :1350-1352 is `++index < rate`), so that is what it means here; with -s it indexes a
     * zero-length table in the reference (undefined behaviour) and is refused.  Rates above 16 (12.8 MS/s) do not fit the
     * demodulation kernel's staging and are refused with a message instead of the usage text. */
    if (cfg.decimation == 0 && !cfg.simultaneous) cfg.decimation = 1;
    if (cfg.decimation == 0 || cfg.decimation > 16) {
        fprintf(stderr, "rtl_wmbus_hip: -d %u: this back end decimates by 1..16 (-d 0 without -s is -d 1)\n", cfg.decimation);
        return EXIT_FAILURE;
    }
    /* -R: a ratio the resampler does not take is a bad option (usage text), decided here without a device */
    if (cfg.input_rate_hz && wmbus_resampler_design(cfg.input_rate_hz, cfg.decimation * 800000u, NULL, NULL, NULL, NULL, 0)) {
        print_usage(argv[0]);
        return EXIT_FAILURE;
    }

    /* -O: beyond half the input rate is a bad option too */
    if (cfg.input_shift_hz && wmbus_shift_design(cfg.input_rate_hz ? cfg.input_rate_hz : cfg.decimation * 800000u, cfg.input_shift_hz, NULL, NULL, 0)) {
        fprintf(stderr, "rtl_wmbus_hip: -O %d: the offset must lie within +- half the input rate (%u Hz)\n", cfg.input_shift_hz,
                (cfg.input_rate_hz ? cfg.input_rate_hz : cfg.decimation * 800000u) / 2u);
        return EXIT_FAILURE;
    }
    for (unsigned ch = 0; ch < cfg.input_channels; ch++)
        if (wmbus_shift_design(cfg.input_rate_hz ? cfg.input_rate_hz : cfg.decimation * 800000u, cfg.input_channel_hz[ch], NULL, NULL, 0)) {
            fprintf(stderr, "rtl_wmbus_hip: -O %d: the offset must lie within +- half the input rate (%u Hz)\n", cfg.input_channel_hz[ch],
                    (cfg.input_rate_hz ? cfg.input_rate_hz : cfg.decimation * 800000u) / 2u);
            return EXIT_FAILURE;
        }

    if (optind < argc) {
        /* batch mode: 2 MiB per file and push (-B overrides).  The staging is page-locked -- files x push bytes (twice that until round 5), pinned by
         * the driver one allocation at a time at about 6 GB/s -- and a job whose files are a few pushes long spends longer
         * pinning than decoding: 1024 files of 64 MiB took 3.9-4.3 s end to end with 8 MiB pushes (16 GB of staging),
         * 2.5-2.7 s with 2 MiB (4 GB), 2.9-3.1 s with 4 MiB; r03, which pinned everything before its first push: 6.6-7.4 s.
         * Round 5 (parallel readers; ONE slab per context, wm_batch.h: the staging is files x push bytes), Gsamples/s decode:
         * 1024 files 20.5-21.3 with 1 MiB, 17-18 with 512-768 KiB, 14.2-15.2 with 2 MiB, 11.5-13.9 with 4 MiB; 512 files 17.5-18.6
         * with 1 MiB, 15.4-15.9 with 2 MiB; 256 files 15.0-15.5 with 1.5-2 MiB, 11.9 with 1 MiB, 14.4-15.7 with 4 MiB
         * (profiles/r05_cli_push_bytes.txt): a context wants 64-128 MiB per push -- less starves the GPU, more makes the
         * pipeline's first and last push, and the pinning, long.  So: 1 MiB per file and push from 384 files per device on, else 2 MiB */
        if (n_devs == 0) { devs[0] = cfg.device; n_devs = 1; }
        if (cfg.max_push_bytes == 0) cfg.max_push_bytes = (argc - optind + n_devs - 1) / n_devs >= 384 ? 1u << 20 : 2u << 20;
        const int rc_batch = run_sharded(cfg, argc - optind, argv + optind, devs, n_devs, map_only, stats);
        if (cfg.crc_repair && cfg.show_algorithm && !map_only) fprintf(stderr, "repair: %llu subjects, %llu repaired\n", repair_subjects, repair_repaired);
        if (cfg.s1_rescue && cfg.show_algorithm && !map_only) fprintf(stderr, "rescue: %llu subjects, %llu rescued\n", rescue_subjects, rescue_rescued);
        if (cfg.line_quality && cfg.show_algorithm && !map_only) fprintf(stderr, "quality: %llu measured, %llu with a closed eye\n", quality_measured, quality_closed);
        finish(rc_batch);
    }
    if (cfg.max_push_bytes == 0) cfg.max_push_bytes = 1u << 20;

    if (check_flow) fprintf(stderr, "rtl_wmbus: monitoring flow\n");
    int fd = 0;
    if (tcp && (fd = open_tcp(tcp)) < 0) return EXIT_FAILURE;

    struct live lv = {NULL, 0, (int)cfg.line_levels, &cfg, 0, {0}, {0}};
    int rc = wmbus_open(&cfg, &lv.ctx);
    if (rc) {
        fprintf(stderr, "rtl_wmbus_hip: cannot open GPU back end: %s\n", lv.ctx ? wmbus_last_error(lv.ctx) : "out of memory");
        wmbus_close(lv.ctx);
        return EXIT_FAILURE;
    }
    /* -f: the reference arms alarm(2) around every fread (rtl_wmbus.c:1300-1302) */
    const wm_reader_cfg rc_cfg = {fd, cfg.max_push_bytes, max_latency_ms, check_flow ? 2000u : 0u};
    if (cfg.channel_activity && census_open(&lv.census, &cfg, 1u, NULL)) { fprintf(stderr, "rtl_wmbus_hip: out of memory\n"); wmbus_close(lv.ctx); return EXIT_FAILURE; }
    const int how = wm_reader_run(&rc_cfg, live_push, &lv);
    if (cfg.channel_activity) { census_resolve(&lv.census, 0, 1u, 0, 1); census_close(&lv.census); }      /* -m: the end of the input resolves the rest */
    if (cfg.input_spectrum && how == WM_READER_EOF) print_spectrum(lv.ctx, 0, &cfg, NULL);
    if (cfg.crc_repair && cfg.show_algorithm) fprintf(stderr, "repair: %llu subjects, %llu repaired\n", repair_subjects, repair_repaired);
    if (cfg.s1_rescue && cfg.show_algorithm) fprintf(stderr, "rescue: %llu subjects, %llu rescued\n", rescue_subjects, rescue_rescued);
    if (cfg.line_quality && cfg.show_algorithm) fprintf(stderr, "quality: %llu measured, %llu with a closed eye\n", quality_measured, quality_closed);
    wmbus_close(lv.ctx);
    if (how == WM_READER_FLOW_STOPPED) {
        fprintf(stderr, "rtl_wmbus: exiting since incoming data stopped flowing!\n");      /* rtl_wmbus.c:76 */
        return EXIT_FAILURE;
    }
    return how == WM_READER_EOF ? EXIT_SUCCESS : EXIT_FAILURE;
}
