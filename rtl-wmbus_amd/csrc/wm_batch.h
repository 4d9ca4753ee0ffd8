/* wm_batch.h -- wmbus_batch_*: many captures on one device (include/wmbus_hip.h).  Part of wm_api.hip's translation unit
 * (it drives the two halves of a push, enqueue_front / enqueue_back and wait_gpu / decode_host, directly).
 *
 * What the headline rate needs lived in bench.py for two rounds: several receiver contexts per GPU, each on its own host
 * thread, free-running through their pushes so that one context's latency-bound framer kernels and host decoding are
 * covered by the other contexts' demodulation kernels (which the library already orders one after the other on the GPU,
 * K1Chain).  It is product code now -- the batch CLI (rtl_wmbus_hip FILE...) and bench.py both go through it -- and it
 * adds one thing a caller of the plain context API cannot do: the NEXT push's front (demodulation, framers) is enqueued
 * BEFORE the previous push is decoded on the host, so host decoding leaves every context's chain of dependent work.
 *
 * Lanes (round 19): where the process has fewer hardware queues than the batch has contexts, streams that share a queue run their
 * pushes one after the other and half the GPU idles.  Neighbouring contexts are then driven as one lane -- one worker thread,
 * one stream, each latency-bound launch carrying the blocks of both (batch_lane_worker, wm_launch.h, wm_lane_merge.h,
 * wm_k_pair.h).  With a queue per context nothing changes. */
#ifndef WM_BATCH_H
#define WM_BATCH_H

struct wmbus_batch {
    wmbus_cfg cfg{};
    char err[256] = {0};
    std::vector<wmbus_ctx *> ctx;
    std::vector<unsigned> first, count;                 /* stream range of every context */
    std::vector<uint8_t *> slab;                        /* per context: its page-locked staging slab (host-sourced runs), allocated on first use */
    std::mutex out_lock, err_lock;
    std::atomic<bool> stop{false};
    int rc = 0;
    bool opened = false;                                /* wmbus_batch_open succeeded: every planned context exists */
    /* Lanes: contexts 2k and 2k + 1, k < pairs, are driven as one lane (one worker thread, one stream, paired launches:
     * batch_lane_worker); every other context is a lane of its own, as before.  pairs = 0 with a hardware queue per context. */
    unsigned pairs = 0;
    unsigned long long last_paired = 0, last_single = 0; /* the last run's kernel launches: two contexts' as one / one context's */
};

namespace {

int batch_fail(wmbus_batch *b, int code, const char *fmt, ...)
{
    std::lock_guard<std::mutex> lk(b->err_lock);
    if (b->rc == 0) {                                       /* the first error is the one reported */
        va_list ap; va_start(ap, fmt);
        vsnprintf(b->err, sizeof b->err, fmt, ap);
        va_end(ap);
        b->rc = code;
    }
    b->stop.store(true);
    return code;
}

struct BatchTotals { std::atomic<uint64_t> samples{0}, lines{0}, paired{0}, single{0}; std::atomic<unsigned> pushes{0}, warnings{0}; };

/* The bytes of context i's next push (0: its input has ended), staged if the run is host-sourced. */
size_t batch_source(wmbus_batch *b, unsigned i, const wmbus_batch_io *io, unsigned &passes_left)
{
    wmbus_ctx *c = b->ctx[i];
    const unsigned S = b->count[i], s0 = b->first[i];
    const size_t pitch = b->cfg.max_push_bytes;
    if (b->stop.load()) return 0;
    if (!io->fill) { if (passes_left == 0) return 0; passes_left--; return io->resident_bytes; }
    /* ONE page-locked slab per context (round 5; two until then): the copies of a push leave the slab long before the next
     * push is read into it -- they were queued an iteration ago and the demodulation kernel behind them has been enqueued
     * since -- so the refill only has to make sure (one event, normally signalled already), and the staging the driver has
     * to pin, at about 5 GB/s and inside the decode time, is files x push bytes instead of twice that. */
    if (!io->self_staged && !b->slab[i]) {
        /* Page-locked staging is allocated HERE, by the context's own thread when it first needs the slab: the driver
         * pins one allocation at a time (16 GB for 1024 files of 8 MiB pushes: 2.4-3 s), so a batch that pinned
         * everything before its first push spent longer setting up than decoding; now the first contexts decode while
         * the others' slabs are still being pinned. */
        hipSetDevice(b->cfg.device);
        if (hipHostMalloc((void **)&b->slab[i], (size_t)S * pitch) != hipSuccess) {
            b->slab[i] = nullptr;
            batch_fail(b, WMBUS_ENOMEM, "batch: cannot allocate %zu bytes of page-locked staging", (size_t)S * pitch);
            return 0;
        }
    }
    if (!io->self_staged && hipEventSynchronize(c->ev_staged) != hipSuccess) { batch_fail(b, WMBUS_EDEVICE, "batch: context %u: waiting for the staging copies failed", i); return 0; }
    const size_t n = io->fill(io->user, s0, S, io->self_staged ? nullptr : b->slab[i], pitch, pitch);
    if (n == 0) return 0;
    if (n > pitch || n % WMBUS_BLOCK_BYTES) { batch_fail(b, WMBUS_EINVAL, "batch: the source returned %zu bytes (multiple of 4096, at most %zu)", n, pitch); return 0; }
    if (!io->self_staged) {
#ifndef WM_STAGE_PER_STREAM
        { const int src = wm_stage_all(c, b->slab[i], pitch, n); if (src) { batch_fail(b, src, "batch: context %u: %s", i, c->err); return 0; } }      /* the code as it came (an argument error is not a device error) */
#else                                                       /* one copy per stream (until round 5; A/B) */
        for (unsigned s = 0; s < S; s++)
            if (wmbus_stage(c, s, b->slab[i] + (size_t)s * pitch, n)) { batch_fail(b, WMBUS_EDEVICE, "batch: context %u: %s", i, c->err); return 0; }
#endif
    }
    return n;
}

/* The previous push of context i: decoded on the host, its lines handed to the sink. */
int batch_deliver(wmbus_batch *b, unsigned i, const wmbus_batch_io *io, BatchTotals *tot)
{
    wmbus_ctx *c = b->ctx[i];
    const unsigned S = b->count[i], s0 = b->first[i];
    const int rc = decode_host(c);
    if (rc) return rc;
    tot->lines += c->lines.size();
    tot->warnings |= c->tim.warnings;
    if (io->lines) {
        /* the lines carry batch-wide stream numbers for the sink (and are put back: the context's own view stays local) */
        for (auto &l : c->lines) l.stream += s0;
        {
            std::lock_guard<std::mutex> lk(b->out_lock);
            io->lines(io->user, s0, S, c->lines.data(), c->lines.size(), c->text.c_str(), &c->tim);
        }
        for (auto &l : c->lines) l.stream -= s0;
    }
    return 0;
}

/* One context's run: pushes until its source ends.  GPU work of push k+1 (front) overlaps the host decode of push k;
 * in host-sourced runs the bytes of push k+1 are read and staged into the context's other input window while push k is
 * in flight. */
void batch_worker(wmbus_batch *b, unsigned i, const wmbus_batch_io *io, BatchTotals *tot)
{
    wmbus_ctx *c = b->ctx[i];
    const unsigned S = b->count[i];
    unsigned passes_left = io->fill ? 0u : io->passes;
    size_t n_cur = batch_source(b, i, io, passes_left);
    bool have_prev = false;
    while (n_cur || have_prev) {                            /* after an error elsewhere the source returns 0: the loop winds down */
        int rc = 0;
        if (n_cur) rc = enqueue_front(c, n_cur);
        if (!rc && have_prev) rc = batch_deliver(b, i, io, tot);
        if (!rc && n_cur) rc = enqueue_back(c);
        if (rc) { batch_fail(b, rc, "batch: context %u: %s", i, c->err); break; }
        const size_t n_next = n_cur ? batch_source(b, i, io, passes_left) : 0;
        if (n_cur) {
            rc = wait_gpu(c);
            if (rc) { batch_fail(b, rc, "batch: context %u: %s", i, c->err); break; }
            tot->samples += (uint64_t)S * (n_cur / k0_bps((int)b->cfg.input_format));
            tot->pushes++;
            have_prev = true;
        } else have_prev = false;
        n_cur = n_next;
    }
    if (c->in_flight) wait_gpu(c);                          /* an aborted run leaves nothing on the stream */
    tot->single += c->n_single;
}

/* A lane's recorded halves leave for its stream: the two lists merged (wm_lane_merge.h), equal pairable kernels as one
 * launch, everything else singly.  `rec[m]` may be empty (a mate whose source has ended, or that has no push in flight). */
int lane_issue(wmbus_batch *b, wmbus_ctx *const cs[2], WmLaneRec rec[2], BatchTotals *tot)
{
    std::vector<WmLaneKey> key[2];
    for (int m = 0; m < 2; m++) for (const WmLaneOp &op : rec[m].ops) key[m].push_back(op.key);
    hipError_t e = hipSuccess;
    const char *what = "";
    int who = 0;
    unsigned long long paired = 0, single = 0;
    wm_lane_merge(key[0].data(), key[0].size(), key[1].data(), key[1].size(), [&](long ia, long ib) {
        if (e != hipSuccess) return;
        if (ia >= 0 && ib >= 0) {
            const WmLaneOp &x = rec[0].ops[(size_t)ia];
            e = x.pair(cs[0]->stream, x, rec[1].ops[(size_t)ib]);
            paired++; what = "paired kernel launch";
        } else {
            who = ia >= 0 ? 0 : 1;
            const WmLaneOp &x = rec[who].ops[(size_t)(ia >= 0 ? ia : ib)];
            e = x.run();
            single += x.launch; what = x.what;
        }
    });
    tot->paired += paired; tot->single += single;
    for (int m = 0; m < 2; m++) rec[m].ops.clear();
    if (wm_turn_held) { wm_turn_held->m.unlock(); wm_turn_held = nullptr; }      /* an operation between the two ends of a K1 turn failed */
    if (e == hipSuccess) return 0;
    for (int m = 0; m < 2; m++) if (cs[m]) cs[m]->poisoned = true;               /* half a push is on the stream */
    (void)b;
    return fail(cs[who], WMBUS_EDEVICE, "%s: %s", what, hipGetErrorString(e));
}

/* A lane: two contexts that would share a hardware queue, driven by ONE thread on ONE stream (wmbus_batch_open has put both
 * on the first one's).  Streams that share a queue run their work one after the other anyway -- whole pushes of one, then
 * of the other --, so at most as many kernels are in flight as there are queues, and the latency-bound framer and burst
 * kernels of a 128-capture context cannot fill the GPU.  The lane makes each of those launches carry both contexts' blocks.
 * The loop is batch_worker's, every step for both mates: fronts recorded and merged; the previous pushes decoded; backs
 * recorded and merged; the sources of the next pushes; wait.  A mate whose source has ended leaves the lane to the other. */
void batch_lane_worker(wmbus_batch *b, unsigned i0, const wmbus_batch_io *io, BatchTotals *tot)
{
    const unsigned idx[2] = {i0, i0 + 1u};
    wmbus_ctx *const cs[2] = {b->ctx[i0], b->ctx[i0 + 1u]};
    WmLaneRec rec[2];
    unsigned passes_left[2];
    size_t n_cur[2], n_next[2];
    bool have_prev[2] = {false, false};
    for (int m = 0; m < 2; m++) { passes_left[m] = io->fill ? 0u : io->passes; n_cur[m] = batch_source(b, idx[m], io, passes_left[m]); }
    /* one half of both mates: listed, then issued; an error stops the lane */
    auto half = [&](bool front) -> int {
        int rc = 0, bad = 0;
        for (int m = 0; m < 2 && !rc; m++) {
            if (!n_cur[m]) continue;
            cs[m]->rec = &rec[m];
            rc = front ? enqueue_front(cs[m], n_cur[m]) : enqueue_back(cs[m]);
            cs[m]->rec = nullptr;
            bad = m;
        }
        if (rc) {                                           /* nothing of this half has reached the stream, but a mate listed before has moved on */
            for (int m = 0; m < 2; m++) { rec[m].ops.clear(); cs[m]->poisoned = true; }
            return batch_fail(b, rc, "batch: context %u: %s", idx[bad], cs[bad]->err);
        }
        rc = lane_issue(b, cs, rec, tot);
        if (rc) for (int m = 0; m < 2; m++) if (cs[m]->err[0]) return batch_fail(b, rc, "batch: context %u: %s", idx[m], cs[m]->err);
        return rc;
    };
    while (n_cur[0] || n_cur[1] || have_prev[0] || have_prev[1]) {
        int rc = half(true);
        for (int m = 0; m < 2 && !rc; m++)
            if (have_prev[m] && (rc = batch_deliver(b, idx[m], io, tot))) batch_fail(b, rc, "batch: context %u: %s", idx[m], cs[m]->err);
        if (!rc) rc = half(false);
        if (rc) break;
        for (int m = 0; m < 2; m++) n_next[m] = n_cur[m] ? batch_source(b, idx[m], io, passes_left[m]) : 0;
        for (int m = 0; m < 2 && !rc; m++) {
            have_prev[m] = false;
            if (!n_cur[m]) continue;
            if ((rc = wait_gpu(cs[m]))) { batch_fail(b, rc, "batch: context %u: %s", idx[m], cs[m]->err); break; }
            tot->samples += (uint64_t)b->count[idx[m]] * (n_cur[m] / k0_bps((int)b->cfg.input_format));
            tot->pushes++;
            have_prev[m] = true;
        }
        if (rc) break;
        for (int m = 0; m < 2; m++) n_cur[m] = n_next[m];
    }
    for (int m = 0; m < 2; m++) {
        if (cs[m]->in_flight) wait_gpu(cs[m]);              /* an aborted run leaves nothing on the stream */
        tot->single += cs[m]->n_single;                     /* the host-driven rounds of wait_gpu launch directly */
    }
}

}  // namespace

extern "C" {

const char *wmbus_batch_last_error(const wmbus_batch *b) { return b ? b->err : "null batch"; }

int wmbus_batch_lane_stats(const wmbus_batch *b, unsigned *lanes, unsigned long long *paired_launches, unsigned long long *single_launches)
{
    if (!b || !b->opened) return WMBUS_EINVAL;
    if (lanes) *lanes = (unsigned)b->ctx.size() - b->pairs;
    if (paired_launches) *paired_launches = b->last_paired;
    if (single_launches) *single_launches = b->last_single;
    return WMBUS_OK;
}
unsigned wmbus_batch_contexts(const wmbus_batch *b) { return b ? (unsigned)b->ctx.size() : 0u; }

wmbus_ctx *wmbus_batch_context(wmbus_batch *b, unsigned i, unsigned *first_stream, unsigned *n_streams)
{
    if (!b || i >= b->ctx.size()) return nullptr;
    if (first_stream) *first_stream = b->first[i];
    if (n_streams) *n_streams = b->count[i];
    return b->ctx[i];
}

void wmbus_batch_close(wmbus_batch *b)
{
    if (!b) return;
    for (size_t i = b->ctx.size(); i-- > 0;) wmbus_close(b->ctx[i]);      /* backwards: a lane's second context runs on the first one's stream */
    for (auto *p : b->slab) if (p) hipHostFree(p);
    delete b;
}

/* How a batch is split (no device needed): the number of contexts and, if `counts` is given, the captures of each. */
unsigned wmbus_batch_plan(const wmbus_cfg *cfg, unsigned contexts, unsigned *counts, unsigned cap)
{
    if (!cfg || cfg->n_streams < 1) return 0;
    const unsigned S = cfg->n_streams;
    /* Contexts of whole 64-capture waves where the batch allows it (the clock kernel's cooperative loads need that); by
     * default 8 of them, at most one per 64 captures: 8 x 128 for the 1024 captures of the headline configuration
     * (4 / 6 / 10 / 12 / 16 contexts measured 96 / 111 / 141 / 120 / 117 against 144 Gsamples/s with 8, DESIGN_HISTORY.md section 8).
     * (rounds 4-5 gave tolerance mode twelve -- the demodulation kernel is a third shorter there and a context's chain of framer launches
     * was the bound: 167 against 162 Gsamples/s.  With the clock recovery in its systolic form the chain is 4 ms shorter and eight are
     * ahead again: 211-212 against 206-209, round 6.) */
    unsigned nctx = contexts ? contexts : std::min(8u, std::max(1u, S / 64u));
    nctx = std::max(1u, std::min(nctx, S));
    /* whole groups of 64 wherever the batch has that many captures per context; a remainder (S not a multiple of 64) rides
     * with the last context, which alone then takes the clock kernel's lane-private load path */
    const unsigned gran = S / 64u >= nctx ? 64u : 1u, units = S / gran, rest = S - units * gran;
    for (unsigned i = 0; i < nctx && counts && i < cap; i++)
        counts[i] = gran * (units / nctx + (i < units % nctx ? 1u : 0u)) + (i + 1 == nctx ? rest : 0u);
    return nctx;
}

int wmbus_batch_open(const wmbus_cfg *cfg, unsigned contexts, wmbus_batch **out)
{
    if (!cfg || !out) return WMBUS_EINVAL;
    *out = nullptr;
    wmbus_runtime_init();                                   /* hardware queues for the contexts' streams, if HIP has not started yet */
    wmbus_batch *b = new wmbus_batch();
    b->cfg = *cfg;
    *out = b;                                               /* the caller reads the message, then closes */
    const unsigned S = cfg->n_streams;
    if (S < 1) return batch_fail(b, WMBUS_EINVAL, "batch: n_streams must be >= 1");
    std::vector<unsigned> plan(S);
    const unsigned nctx = wmbus_batch_plan(cfg, contexts, plan.data(), S);
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 16;
    /* the contexts are opened side by side (round 6: one after the other it was 0.06 s each -- allocations, page-locked result areas,
     * initial fills --, 0.3 s of a 320-file batch that decodes in 0.23 s) */
    /* Lanes.  The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (HIP's own default: 4), and streams that share
     * a queue run one after the other: with fewer queues than contexts, neighbours in the plan share a lane instead -- one
     * stream, launches that carry both (batch_lane_worker).  A lane holds two contexts at most: what pairs is paired, the
     * rest run alone.  The caller's GPU_MAX_HW_QUEUES is read, never changed; WMBUS_BATCH_LANES=N overrides the lane count
     * (A/B runs, tests): N >= the number of contexts is one lane, one stream and one worker per context. */
    unsigned lanes = 4;
    if (const char *q = getenv("GPU_MAX_HW_QUEUES")) { const long v = strtol(q, nullptr, 10); if (v >= 1) lanes = (unsigned)std::min(v, 1024L); }
    if (const char *q = getenv("WMBUS_BATCH_LANES")) { const long v = strtol(q, nullptr, 10); if (v >= 1) lanes = (unsigned)std::min(v, 1024L); }
    lanes = std::min(lanes, nctx);
    b->pairs = std::min(nctx - lanes, nctx / 2u);
    std::vector<wmbus_ctx *> opened(nctx, nullptr);
    std::vector<int> rcs(nctx, 0);
    /* first every lane's first context, side by side; then the second ones, each onto its mate's stream */
    for (int second = 0; second < 2; second++) {
        std::vector<std::thread> openers;
        for (unsigned i = 0; i < nctx; i++) {
            const bool mate = i < 2u * b->pairs && (i & 1u);
            if (mate != (second != 0) || (mate && rcs[i - 1u])) continue;
            openers.emplace_back([&, i, mate] {
                wmbus_cfg cc = *cfg;
                cc.n_streams = plan[i];
                /* host decoder threads: the contexts decode at different times, so the box is shared 2 x oversubscribed */
                if (cc.host_threads == 0) cc.host_threads = std::max(2u, std::min(16u, 2u * hw / std::max(1u, nctx)));
                wm_open_on_stream = mate ? opened[i - 1u]->stream : nullptr;
                rcs[i] = wmbus_open(&cc, &opened[i]);
                wm_open_on_stream = nullptr;
            });
        }
        for (auto &t : openers) t.join();
    }
    for (unsigned i = 0; i < nctx; i++)
        if (rcs[i]) {
            batch_fail(b, rcs[i], "batch: context %u of %u (%u captures): %s", i, nctx, plan[i], opened[i] ? opened[i]->err : "out of memory");
            for (size_t k = opened.size(); k-- > 0;) wmbus_close(opened[k]);
            return rcs[i];
        }
    unsigned at = 0;
    for (unsigned i = 0; i < nctx; i++) {
        b->ctx.push_back(opened[i]); b->first.push_back(at); b->count.push_back(plan[i]);
        at += plan[i];
    }
    b->slab.assign(nctx, nullptr);
    b->opened = true;
    return WMBUS_OK;
}

static int batch_locate(wmbus_batch *b, unsigned stream, unsigned *i)
{
    if (!b || !b->opened || stream >= b->cfg.n_streams) return WMBUS_EINVAL;      /* a handle whose open failed has no contexts */
    unsigned k = 0;
    while (k + 1 < b->ctx.size() && stream >= b->first[k + 1]) k++;
    *i = k;
    return WMBUS_OK;
}

int wmbus_batch_stage(wmbus_batch *b, unsigned stream, const uint8_t *cu8, size_t nbytes)
{
    unsigned i;
    if (batch_locate(b, stream, &i)) return WMBUS_EINVAL;
    const int rc = wmbus_stage(b->ctx[i], stream - b->first[i], cu8, nbytes);
    if (rc) { std::lock_guard<std::mutex> lk(b->err_lock); snprintf(b->err, sizeof b->err, "batch: context %u: %s", i, b->ctx[i]->err); }
    return rc;
}

void *wmbus_batch_device_input(wmbus_batch *b, unsigned stream)
{
    unsigned i;
    if (batch_locate(b, stream, &i)) return nullptr;
    return wmbus_device_input(b->ctx[i], stream - b->first[i]);
}

size_t wmbus_batch_line_levels(const wmbus_batch *b, unsigned first_stream, const wmbus_level **levels)
{
    if (levels) *levels = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_line_levels(b->ctx[i], levels);
    return 0;
}

size_t wmbus_batch_line_power(const wmbus_batch *b, unsigned first_stream, const wmbus_power **power)
{
    if (power) *power = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_line_power(b->ctx[i], power);
    return 0;
}

size_t wmbus_batch_activity(const wmbus_batch *b, unsigned first_stream, const wmbus_burst **records)
{
    if (records) *records = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_activity(b->ctx[i], records);
    return 0;
}

size_t wmbus_batch_line_repairs(const wmbus_batch *b, unsigned first_stream, const wmbus_repair **records)
{
    if (records) *records = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_line_repairs(b->ctx[i], records);
    return 0;
}

size_t wmbus_batch_line_rescues(const wmbus_batch *b, unsigned first_stream, const wmbus_rescue **records)
{
    if (records) *records = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_line_rescues(b->ctx[i], records);
    return 0;
}

size_t wmbus_batch_line_quality(const wmbus_batch *b, unsigned first_stream, const wmbus_quality **records)
{
    if (records) *records = nullptr;
    if (!b || !b->opened) return 0;
    for (size_t i = 0; i < b->ctx.size(); i++)
        if (b->first[i] == first_stream) return wmbus_line_quality(b->ctx[i], records);
    return 0;
}

int wmbus_batch_run(wmbus_batch *b, const wmbus_batch_io *io, wmbus_batch_stats *stats)
{
    if (!b || !io) return WMBUS_EINVAL;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!b->opened) return WMBUS_EINVAL;                    /* wmbus_batch_open failed: the handle only carries its message */
    { std::lock_guard<std::mutex> lk(b->err_lock); b->rc = 0; b->err[0] = 0; }
    b->stop.store(false);
    if (!io->fill && (io->resident_bytes == 0 || io->resident_bytes > b->cfg.max_push_bytes || io->resident_bytes % WMBUS_BLOCK_BYTES))
        return batch_fail(b, WMBUS_EINVAL, "batch: resident_bytes must be a positive multiple of 4096 and <= max_push_bytes");
    if (io->fill && b->cfg.input_windows != 2) return batch_fail(b, WMBUS_EINVAL, "batch: a host-sourced run needs cfg.input_windows = 2");
    BatchTotals tot;
    const double t0 = now_ms();
    for (wmbus_ctx *c : b->ctx) c->n_single = 0;
    std::vector<std::thread> th;
    auto lane = [&](unsigned i) { if (i < 2u * b->pairs) batch_lane_worker(b, i, io, &tot); else batch_worker(b, i, io, &tot); };
    for (unsigned i = b->pairs ? 2u : 1u; i < b->ctx.size(); i += i < 2u * b->pairs ? 2u : 1u) th.emplace_back(lane, i);
    lane(0);                                                /* the caller's thread drives the first lane */
    for (auto &t : th) t.join();
    b->last_paired = tot.paired.load(); b->last_single = tot.single.load();
    if (stats) {
        stats->seconds = (now_ms() - t0) * 1e-3;
        stats->samples = tot.samples.load(); stats->lines = tot.lines.load(); stats->pushes = tot.pushes.load(); stats->warnings = tot.warnings.load();
    }
    return b->rc;
}

}  // extern "C"

#endif /* WM_BATCH_H */
