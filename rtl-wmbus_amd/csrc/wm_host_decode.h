/* wm_host_decode.h -- the host half of wmbus_collect: candidate telegrams in pinned host memory -> datagram lines (sort, the reference's
 * "busy decoder ignores an access code" rule, strip + format, persistent plain-C decoders for bursts cut by a push boundary, merge in the reference's
 * stdout order).  Part of wm_api.hip's translation unit (it reads wmbus_ctx); no HIP call: the next push's front may be on the GPU while it runs. */
#ifndef WM_HOST_DECODE_H
#define WM_HOST_DECODE_H

namespace {

/* one formatted line of a push: where its text lies in its part's buffer (round 6: a std::string per line was a heap allocation per
 * line -- with eight ranks' contexts decoding at once on one host, 64 x 4 threads in malloc, the decode of a context-push took
 * 18 ms instead of 2.8: tools/host_replay.py) */
struct LineRec {
    uint64_t sample; uint32_t stream; uint8_t chain, algo, crc_ok; uint32_t seq; uint32_t part, off, len;
    uint32_t lev;              /* cfg.line_levels: its level record in its part's `levs` */
};
struct LinePart { std::vector<LineRec> recs; std::string text; std::vector<wmbus_level> levs; std::vector<wmbus_repair> reps; std::vector<wmbus_quality> quals; std::vector<wmbus_rescue> ress;
                  unsigned res_subjects = 0, res_rescued = 0; };   /* reps: cfg.crc_repair, quals: cfg.line_quality, ress: cfg.s1_rescue (and its counts), beside levs */

/* Persistent host worker pool of a context (packet decoders): run(n, f) executes f(0..n-1) on the
 * workers and the caller; threads are created once, not per push. */
class WorkerPool {
public:
    explicit WorkerPool(unsigned n_workers)
    {
        for (unsigned i = 0; i < n_workers; i++) th_.emplace_back([this] { loop(); });
    }
    ~WorkerPool()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    unsigned size() const { return (unsigned)th_.size(); }
    template <typename F> void run(unsigned n, F &&f)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = f; next_ = 0; total_ = n; done_ = 0; gen_++;      /* the job lives in the pool, not on this stack frame */
        }
        cv_.notify_all();
        work();                                              /* the caller helps */
        std::unique_lock<std::mutex> lk(m_);
        /* every item done AND every worker that picked this generation up has left work(): nothing of
         * this run can still be executing when the caller's captures go out of scope */
        cv_done_.wait(lk, [&] { return done_ == total_ && active_ == 0; });
        job_ = nullptr;
    }
private:
    void work()
    {
        for (;;) {
            unsigned i;
            { std::lock_guard<std::mutex> lk(m_); if (next_ >= total_) return; i = next_++; }
            job_(i);                                         /* job_ only changes while no item is outstanding */
            { std::lock_guard<std::mutex> lk(m_); if (++done_ == total_) cv_done_.notify_all(); }
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || (gen_ != seen && job_ != nullptr); });
                if (stop_) return;
                seen = gen_; active_++;
            }
            work();
            { std::lock_guard<std::mutex> lk(m_); if (--active_ == 0) cv_done_.notify_all(); }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, cv_done_;
    std::function<void(unsigned)> job_;
    unsigned next_ = 0, total_ = 0, done_ = 0, active_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

struct Entry { uint32_t idx; uint8_t raw; };          /* one candidate telegram of a push: a WmPkt (decoded on the GPU) or a WmBurstHdr (chips) */
struct EntryKey { uint32_t stream, chip0; uint8_t chain, algo, cont; };

}  // namespace

static EntryKey entry_key(const wmbus_ctx *c, const Entry &e)
{
    if (e.raw) { const WmBurstHdr &h = c->h_hdr[e.idx]; return EntryKey{h.stream, h.chip0, h.chain, h.algo, (uint8_t)(h.flags & 1u)}; }
    const WmPkt &p = c->h_pkts[e.idx];
    return EntryKey{p.stream, p.chip0, p.chain, p.algo, 0};
}

/* TIMESTAMP field of a line.  The reference stamps a telegram when its last chip is processed (t1_c1_packet_decoder.h:
 * 390,458, s1_packet_decoder.h:229), which behind a live SDR is the moment that sample arrived.  A push is handed over
 * when its LAST sample has arrived, so a telegram completed by decimated sample m of the push was on the air
 * (m_end - 1 - m) / 800 kHz earlier (the decimated rate is 800 kS/s whatever -d is, rtl_wmbus.c:1296). */
static void line_timestamp(const wmbus_ctx *c, uint64_t sample, const char *ts_fixed, char *ts, size_t cap)
{
    if (ts_fixed) { snprintf(ts, cap, "%s", ts_fixed); return; }
    const uint64_t back = c->done.m_end > sample ? c->done.m_end - 1u - sample : 0u;
    const int64_t us = (int64_t)c->done.arrival.tv_sec * 1000000 + c->done.arrival.tv_usec - (int64_t)(back * 5u / 4u);   /* 1.25 us per decimated sample */
    wm_timestamp_at(ts, cap, (long)(us / 1000000), (long)(us % 1000000));
}

/* Candidate telegrams of the (stream, chain, framer) groups in order[lo, hi), each group in chip order: what the
 * reference's decoder would do with them -- an access code that passes while the decoder is busy is ignored
 * (t1_c1_packet_decoder.h:272-278), a telegram the GPU has assembled is stripped and formatted, a burst cut by the end
 * of the push goes chip by chip through the persistent host decoder. */
static void decode_stream_range(wmbus_ctx *c, const std::vector<Entry> &order, size_t lo, size_t hi,
                                LinePart &part, uint32_t part_no, const char *ts_fixed)
{
    std::vector<LineRec> &out = part.recs;
    /* the level travels with its item to the line it produces: a packet's is record idx of h_lev_pkts, a burst's the one its decoder keeps */
    /* the repair record likewise (cfg.crc_repair switches the levels on: the two vectors run in step): a packet's is record idx of
     * h_rep_pkts, a burst the host decoders finished was no subject */
    /* and the quality record (cfg.line_quality): record idx of h_q_pkts, n = 0 for a burst the host decoders finished */
    /* and the rescue record (cfg.s1_rescue): record idx of h_res_pkts for a rescued line, zero for every other */
    auto keep = [&](LineRec &r, const char *line, size_t n, const wmbus_level *lev, const wmbus_repair *rep, const wmbus_quality *ql, const wmbus_rescue *rs = nullptr) {
        r.part = part_no; r.off = (uint32_t)part.text.size(); r.len = (uint32_t)n;
        r.lev = (uint32_t)part.levs.size();
        if (c->lev_on) part.levs.push_back(*lev);
        if (c->rep_on) part.reps.push_back(rep ? *rep : wmbus_repair{});
        if (c->q_on) part.quals.push_back(ql ? *ql : wmbus_quality{});
        if (c->res_on) part.ress.push_back(rs ? *rs : wmbus_rescue{});
        part.text.append(line, n);
        out.push_back(r);
    };
    char line[1024], ts[64];
    uint8_t pkt[WM_PKT_MAXBYTES + 4];
    uint32_t seq = 0;
    size_t i = lo;
    while (i < hi) {
        const EntryKey k0 = entry_key(c, order[i]);
        HostDecoder &hd = c->decs[((size_t)k0.stream * 2 + k0.chain) * 2 + k0.algo];
        const char *tag = c->cfg.show_algorithm ? (k0.algo == WMBUS_ALGO_RLA ? "rla;" : "t2a;") : "";
        uint64_t next_free = 0;                         /* first chip the decoder has not consumed */
        size_t j = i;
        for (; j < hi; j++) {
            const EntryKey kj = entry_key(c, order[j]);
            if (kj.stream != k0.stream || kj.chain != k0.chain || kj.algo != k0.algo) break;
            if (!order[j].raw) {
                /* ---- the whole burst was inside the push: the GPU has run the decoder over it ---- */
                const WmPkt &p = c->h_pkts[order[j].idx];
                if (hd.owed != 0 || p.chip0 < next_free) continue;     /* the access code passed while the decoder was busy */
                next_free = (uint64_t)p.chip0 + p.consumed;
                if (c->res_on && p.status == WM_PKT_ABORT) {
                    /* cfg.s1_rescue: the decoder took this access code and gave up, as ever (next_free above is the abort's); k3_rescue
                     * has decoded the telegram after all where the flag says so */
                    const wmbus_rescue &rs = c->h_res_pkts[order[j].idx];
                    if (rs.status) { part.res_subjects++; part.res_rescued += rs.status == 1u; }
                    if (p.flags & WM_PKTF_RESCUED) {
                        const unsigned nb = std::min<unsigned>(std::max<unsigned>(p.L, 2u), WM_PKT_MAXBYTES);
                        memset(pkt, 0, sizeof pkt);
                        memcpy(pkt, c->h_bytes + p.off, nb);
                        line_timestamp(c, p.sample, ts_fixed, ts, sizeof ts);
                        const size_t n = wm_packet_format(WM_MODE_S1, 0, 0, 0, 1, p.L, pkt, p.pkt_rssi, p.rssi_now, tag, ts, line, sizeof line);
                        LineRec r; r.sample = p.sample; r.stream = p.stream; r.chain = p.chain; r.algo = p.algo;
                        r.crc_ok = 1; r.seq = seq++;
                        keep(r, line, n, c->lev_on ? &c->h_lev_pkts[order[j].idx] : nullptr, nullptr, nullptr, &rs);
                    }
                }
                if (p.status != WM_PKT_DONE) continue;
                const unsigned nb = std::min<unsigned>(std::max<unsigned>(p.L, 2u), WM_PKT_MAXBYTES);
                /* the reference's decoder is memset on reset (t1_c1_packet_decoder.h:268,276): bytes a short telegram never
                 * stored read as zero in the ident field of its line (get_serial looks at bytes 4..7 whatever L is) */
                memset(pkt, 0, sizeof pkt);
                memcpy(pkt, c->h_bytes + p.off, nb);
                line_timestamp(c, p.sample, ts_fixed, ts, sizeof ts);
                const int ok = (p.flags & WM_PKTF_CRC_OK) != 0;
                const size_t n = wm_packet_format(p.chain ? WM_MODE_S1 : WM_MODE_T1C1, (p.flags & WM_PKTF_C1) != 0, (p.flags & WM_PKTF_FRAME_B) != 0,
                                                  (p.flags & WM_PKTF_ERR3OF6) != 0, ok, p.L, pkt, p.pkt_rssi, p.rssi_now, tag, ts, line, sizeof line);
                LineRec r; r.sample = p.sample; r.stream = p.stream; r.chain = p.chain; r.algo = p.algo;
                r.crc_ok = (uint8_t)ok; r.seq = seq++;
                keep(r, line, n, c->lev_on ? &c->h_lev_pkts[order[j].idx] : nullptr, c->rep_on ? &c->h_rep_pkts[order[j].idx] : nullptr,
                     c->q_on ? &c->h_q_pkts[order[j].idx] : nullptr);
                continue;
            }
            const WmBurstHdr &h = c->h_hdr[order[j].idx];
            const bool cont = h.flags & 1u;
            if (cont ? hd.owed == 0 : (hd.owed != 0 || h.chip0 < next_free)) continue;   /* the access code passed while the decoder was busy */
            if (c->lev_on && !cont) hd.lev = c->h_lev_hdr[order[j].idx];      /* the decoder takes this burst: its level stays with it until the line, in a later push if need be */
            const uint32_t *w = c->h_words + h.word_off;
            int st = cont ? WM_DEC_RECEIVING : WM_DEC_IDLE;
            uint32_t k = 0;
            for (; k < h.n_chips; k++) {
                const uint32_t word = w[k];
                const unsigned val = word & 7u, rssi = (word >> 3) & 0xFFu;
                if ((val & 4u) && st == WM_DEC_RECEIVING) {   /* the run-length framer reset itself: telegram lost */
                    wm_decoder_abort(&hd.dec);
                    st = WM_DEC_IDLE;
                    break;                                     /* this chip may start a burst of its own */
                }
                st = wm_decoder_chip(&hd.dec, val & 3u, rssi);
                if (st == WM_DEC_DONE) {
                    int ok = 0;
                    line_timestamp(c, h.pos0 + (word >> 11), ts_fixed, ts, sizeof ts);
                    const size_t n = wm_decoder_format(&hd.dec, tag, ts, rssi, line, sizeof line, &ok);
                    LineRec r; r.sample = h.pos0 + (word >> 11); r.stream = h.stream; r.chain = h.chain; r.algo = h.algo;
                    r.crc_ok = (uint8_t)ok; r.seq = seq++;
                    keep(r, line, n, &hd.lev, nullptr, nullptr);
                    st = WM_DEC_IDLE;
                }
                if (st == WM_DEC_IDLE) { k++; break; }
            }
            next_free = (uint64_t)h.chip0 + k;
            const bool cut = st == WM_DEC_RECEIVING;
            if (cut && h.n_chips != h.avail) {                 /* device under-estimated the burst: a bug */
                uint32_t none = 0;
                c->short_burst.compare_exchange_strong(none, 1u + order[j].idx);
            }
            hd.owed = cut ? std::max(1u, wm_decoder_chips_owed(&hd.dec)) : 0u;
            hd.fed = c->done.seq;
        }
        i = j;
    }
}

/* Second half: candidate telegrams -> lines (host packet decoders, strip, format, merge).  Touches pinned host memory
 * and the decoders only, so the NEXT push's front may already be on the GPU. */
static int decode_host(wmbus_ctx *c)
{
    c->lines.clear(); c->text.clear(); c->levels.clear(); c->powers.clear(); c->repairs.clear(); c->rescues.clear(); c->res_subjects = c->res_rescued = 0; c->qualities.clear();
    c->short_burst.store(0);
    if (!c->done.valid) return WMBUS_OK;
    c->done.valid = false;
    const double t0 = now_ms();
    const uint32_t n_hdr = c->done.n_hdr, n_pkts = c->done.n_pkts;

    /* candidates in the order the decoders take them: (capture, chain, framer), a continuation first, then by chip.  The key is made
     * ONCE per candidate (the comparator used to look every candidate's record up in the page-locked result area at every comparison) */
    std::vector<Entry> order(n_hdr + n_pkts);
    {
        struct Keyed { uint64_t hi; uint32_t lo; Entry e; };
        std::vector<Keyed> ks(n_hdr + n_pkts);
        for (uint32_t i = 0; i < n_hdr + n_pkts; i++) {
            const Entry e = i < n_hdr ? Entry{i, 1} : Entry{i - n_hdr, 0};
            const EntryKey k = entry_key(c, e);
            ks[i] = Keyed{((uint64_t)k.stream << 8) | ((uint64_t)k.chain << 4) | ((uint64_t)k.algo << 1) | (k.cont ? 0u : 1u), k.chip0, e};
        }
        std::stable_sort(ks.begin(), ks.end(), [](const Keyed &x, const Keyed &y) { return x.hi != y.hi ? x.hi < y.hi : x.lo < y.lo; });
        for (size_t i = 0; i < ks.size(); i++) order[i] = ks[i].e;
    }
    unsigned nt = c->cfg.host_threads ? c->cfg.host_threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (order.size() < 4096) nt = 1;
    const char *tsf = c->cfg.fixed_timestamp ? "TS" : nullptr;
    /* more pieces than threads (cut at stream boundaries): the decoders' cost per stream is uneven */
    const unsigned np = nt == 1 ? 1 : 4 * nt;
    std::vector<LinePart> parts(np);
    if (np == 1) decode_stream_range(c, order, 0, order.size(), parts[0], 0u, tsf);
    else {
        std::vector<size_t> cut(np + 1, order.size());
        cut[0] = 0;
        for (unsigned t = 1; t < np; t++) {
            size_t p = order.size() * t / np;
            while (p < order.size() && p > 0 && entry_key(c, order[p]).stream == entry_key(c, order[p - 1]).stream) p++;
            cut[t] = std::max(p, cut[t - 1]);
        }
        if (!c->pool || c->pool->size() + 1 != nt) c->pool.reset(new WorkerPool(nt - 1));
        c->pool->run(np, [&](unsigned t) { decode_stream_range(c, order, cut[t], cut[t + 1], parts[t], t, tsf); });
    }
    /* Burst storage ran out (a warning): a half-received telegram whose continuation was among the dropped bursts would
     * otherwise wait for it for ever and take the FIRST chips of the next push for its own -- it is lost, like the
     * bursts that were dropped. */
    if (c->tim.warnings & WMBUS_WARN_BURSTS_DROPPED)
        for (auto &hd : c->decs)
            if (hd.owed != 0 && hd.fed != c->done.seq) { wm_decoder_abort(&hd.dec); hd.owed = 0; }
    for (auto &p : parts) { c->res_subjects += p.res_subjects; c->res_rescued += p.res_rescued; }
    /* stdout order of the reference: by completing sample, then T1/C1 before S1, run-length before time2 */
    std::vector<LineRec> all;
    {
        size_t n_all = 0, n_text = 0;
        for (auto &p : parts) { n_all += p.recs.size(); n_text += p.text.size(); }
        all.reserve(n_all); c->text.reserve(n_text); c->lines.reserve(n_all);
        for (auto &p : parts) all.insert(all.end(), p.recs.begin(), p.recs.end());
    }
    std::stable_sort(all.begin(), all.end(), [](const LineRec &a, const LineRec &b) {
        if (a.stream != b.stream) return a.stream < b.stream;
        if (a.sample != b.sample) return a.sample < b.sample;
        if (a.chain != b.chain) return a.chain < b.chain;
        if (a.algo != b.algo) return a.algo < b.algo;
        return a.seq < b.seq;
    });
    /* Options (off by default: the drop-in prints what the reference prints).  Both framers work on every burst, so a
     * clean telegram is printed twice, once per framer (README.md:105-108 "You will eventually get two identical
     * datagrams"): dedup_twins drops the later of two lines of one capture and mode that carry the same payload, come
     * from different framers and complete within one longest-telegram time of each other.  only_crc_ok drops what a
     * consumer like wmbusmeters would discard anyway. */
    if (c->cfg.dedup_twins || c->cfg.only_crc_ok) {
        if (c->twins.empty()) c->twins.assign((size_t)c->S * 2 * 2, wm_twin{0, 0, 0, 0});
        std::vector<LineRec> kept;
        kept.reserve(all.size());
        for (auto &r : all) {
            if (c->cfg.only_crc_ok && !r.crc_ok) continue;
            if (c->cfg.dedup_twins && wm_twin_check(&c->twins[((size_t)r.stream * 2 + r.chain) * 2], r.chain, r.algo, r.sample, parts[r.part].text.data() + r.off, r.len)) continue;
            kept.push_back(r);
        }
        all.swap(kept);
    }
    std::vector<uint32_t> pw_scratch;
    for (auto &r : all) {
        wmbus_line l{};
        /* r.stream is the pipeline stream v = capture * CH + channel (the sort above: captures ascending, channels within a capture) */
        l.stream = r.stream / c->CH; l.channel = (uint8_t)(r.stream % c->CH);
        l.chain = r.chain; l.algo = r.algo; l.crc_ok = r.crc_ok; l.sample = r.sample;
        l.text_off = (uint32_t)c->text.size(); l.text_len = r.len;
        c->text.append(parts[r.part].text, r.off, r.len);
        c->lines.push_back(l);
        if (c->lev_on) c->levels.push_back(parts[r.part].levs[r.lev]);
        if (c->rep_on) c->repairs.push_back(parts[r.part].reps[r.lev]);
        if (c->q_on) c->qualities.push_back(parts[r.part].quals[r.lev]);
        if (c->res_on) c->rescues.push_back(parts[r.part].ress[r.lev]);
        if (c->pw.on) {
            /* cfg.line_power: the line's record from its row's P history (wm_k0_power.h).  Its access-code sample came with the level record
             * -- for a burst finished in a later push the decoder kept it -- its completing sample is the line's; both are decimated
             * samples of the pipeline's stream, m(n) = floor(n D M / L) the raw input sample they stand for. */
            const std::vector<uint32_t> &p = c->pw.ring[(size_t)r.chain * c->S + r.stream];
            const uint64_t ka = k0_pow_block_of(parts[r.part].levs[r.lev].sync_sample, c->d, c->k0.L, c->k0.M), ke = k0_pow_block_of(r.sample, c->d, c->k0.L, c->k0.M);
            wmbus_power rec{};
            power_record(&rec, k0_line_power_rule(p.data(), c->pw.ring_first, p.size(), ka, ke, c->pw.fin, pw_scratch));
            c->powers.push_back(rec);
        }
    }
    c->tim.host_decode_ms = (float)(now_ms() - t0);
    if (const uint32_t sb = c->short_burst.load()) {       /* formatted once, after the pool has joined */
        const WmBurstHdr &h = c->h_hdr[sb - 1u];
        return fail(c, WMBUS_EDEVICE, "burst too short: stream %u chain %u algo %u chip %u", h.stream, h.chain, h.algo, h.chip0);
    }
    return WMBUS_OK;
}

#endif /* WM_HOST_DECODE_H */
