"""S1 rescue on the GPU (cfg.s1_rescue): through the C ABI the lines, wmbus_line.crc_ok, the rescue records and the stats equal
tests/rescue_ref.py on the oracle's taps and chips -- on the two synthetic S1 captures, under the switches that change how a burst
reaches the burst kernel, cut into pushes, beside -s, beside crc_repair and line_quality, through a batch's sink and the CLI; every line
that is no rescue is the line of a context without the field, in the same order; and a context without the field is the one it was.
The tests that compare against rescue_capture fail on a tree without the feature."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rescue_ref as RF
import telegram_ref as TR
from lanes import one_lane

pytestmark = pytest.mark.gpu

PUSH_SAMPLES = 1 << 16                                      # the cut of the push test, input samples
CONFIGS = {"product": dict(keep_taps=False), "debug-views": dict(keep_taps=True), "one-wave-clock": dict(keep_taps=False, clock_waves=1),
           "systolic-clock": dict(keep_taps=False, clock_waves=4), "rounds-on-host": dict(keep_taps=False, rounds_on_host=True)}


@pytest.fixture(scope="module")
def captures(oracle):
    """The two captures, the oracle's run of each and what the restatement makes of it: computed once, shared, left unchanged."""
    out = {}
    for name in RF.SYNTHETIC:
        cu8, sent = RF.synthetic(name)
        ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
        out[name] = dict(cu8=cu8, ref=ref, want=RF.rescue_capture(ref), cut=RF.rescue_capture(ref, push_m=PUSH_SAMPLES // 2), sent=sent)
    return out


def run(wm, cu8, sizes=None, **kw):
    """([(line dict, rescue dict or None)], (subjects, rescued) summed over the pushes) of one capture over the pushes `sizes` (bytes)."""
    kw.setdefault("s1_rescue", 1)
    sizes = sizes or [cu8.size]
    out, stats = [], [0, 0]
    with wm.Receiver(n_streams=1, max_push_bytes=max(sizes), **kw) as rx:
        off = 0
        for n in sizes:
            rx.push([cu8[off:off + n]]); off += n
            lines, recs = rx.lines(), rx.line_rescues()
            assert len(recs) == (len(lines) if kw["s1_rescue"] else 0)
            out += [(ln, recs[k] if recs else None) for k, ln in enumerate(lines)]
            s, r = rx.rescue_stats()
            stats[0] += s; stats[1] += r
    return out, tuple(stats)


def check(got, want):
    """Byte for byte: the text, crc_ok, the records, the stats."""
    got, stats = got
    assert [ln["text"] for ln, _ in got] == want["lines"]
    assert [ln["crc_ok"] for ln, _ in got] == want["crc_ok"]
    assert [rp for _, rp in got] == want["records"]
    assert stats == want["stats"]


def rotated(cu8, hz=-325e3):
    """The capture moved `hz` from the centre (1.6 MS/s): -s looks for S1 325 kHz below it."""
    x = (cu8.astype(np.float64) - 127.5).reshape(-1, 2)
    z = (x[:, 0] + 1j * x[:, 1]) * np.exp(2j * np.pi * hz / 1.6e6 * np.arange(x.shape[0]))
    return np.clip(np.rint(np.stack([z.real, z.imag], 1) + 127.5), 0, 255).astype(np.uint8).reshape(-1)


def conditions(c):
    """What the issue asks of a capture, so that one that rescues nothing cannot pass silently."""
    n = RF.counts(c["want"], c["sent"])
    assert n["rescued"] >= 3 and (n["gated"] >= 1 or n["bad"] >= 1) and n["decoded"] >= 1 and n["false_rescues"] == 0, n


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(RF.SYNTHETIC))
def test_against_the_restatement(wm, captures, name, config):
    c = captures[name]
    conditions(c)
    got = run(wm, c["cu8"], **CONFIGS[config])
    check(got, c["want"])
    sent = {TR.printed_hex(False, a, len(a)) for a in c["sent"]}
    for (ln, rp), rescued in zip(got[0], c["want"]["rescued"]):
        assert (rp["status"] == 1) == rescued
        if rescued:                                         # no false rescue: a rescued line carries a telegram that was sent
            assert ln["text"].startswith("t2a;S1;1;1;") and ln["text"].rstrip().split(";0x")[1] in sent and ln["chain"] == 1 and ln["algo"] == 1


@pytest.mark.parametrize("name", list(RF.SYNTHETIC))
def test_push_cuts(wm, captures, name):
    """Pushes of 2^16 samples: a subject inside a push is rescued as in the single push; a telegram that straddles a push edge is finished
    or aborted by the host decoders and keeps today's output -- no line."""
    c = captures[name]
    total = c["cu8"].size
    sizes = [min(2 * PUSH_SAMPLES, total - off) for off in range(0, total, 2 * PUSH_SAMPLES)]
    got = run(wm, c["cu8"], sizes, keep_taps=False)
    check(got, c["cut"])
    one, cut = c["want"], c["cut"]
    assert cut["stats"][1] < one["stats"][1]                # the cut does cost a rescue
    assert [ln for ln, r in zip(cut["lines"], cut["rescued"]) if not r] == c["ref"]["text"].splitlines(keepends=True)
    assert set(ln for ln, r in zip(cut["lines"], cut["rescued"]) if r) <= set(ln for ln, r in zip(one["lines"], one["rescued"]) if r)
    print(name, "rescued in one push", one["stats"], "cut into pushes", cut["stats"])


@pytest.mark.parametrize("name", list(RF.SYNTHETIC))
def test_field_off_and_every_other_line_unchanged(wm, captures, name):
    c = captures[name]
    off, _ = run(wm, c["cu8"], keep_taps=False, s1_rescue=0)
    assert "".join(ln["text"] for ln, _ in off) == c["ref"]["text"]
    on, _ = run(wm, c["cu8"], keep_taps=False)
    assert [ln for ln, rp in on if rp["status"] != 1] == [ln for ln, _ in off]         # the whole line records, in the same order
    with wm.Receiver(n_streams=1, max_push_bytes=c["cu8"].size, keep_taps=False) as rx:
        assert rx.cfg.s1_rescue == 0
        rx.push([c["cu8"]])
        p = ctypes.POINTER(wm.Rescue)()
        assert rx.lines_count() == len(off) and wm.lib().wmbus_line_rescues(rx._h, ctypes.byref(p)) == 0 and not p
        assert wm.lib().wmbus_rescue_stats(rx._h, None, None) == -1 and rx.rescue_stats() == (0, 0)
        assert rx.line_levels() == []                       # the field's own switch-on of the level records is not there either


def test_beside_simultaneous(wm, oracle, captures):
    """-s looks for S1 325 kHz below the centre: the capture rotated there, the restatement on the oracle's -s run of it."""
    cu8 = rotated(captures["s1-l40"]["cu8"])
    ref = oracle.run(cu8, oracle.make_opts(simultaneous=1), taps=True, chips=True)
    want = RF.rescue_capture(ref)
    assert want["stats"][1] >= 3
    check(run(wm, cu8, simultaneous=True, keep_taps=False), want)
    print("-s: stats", want["stats"], "gated", want["gated"])


def test_beside_repair_and_quality(wm, captures):
    """crc_repair = 1 and line_quality = 1 together with the field: the same lines and rescue records; a rescued line's repair and quality
    records are zero (those kernels saw an abort), every other line's are those of the context without s1_rescue."""
    c = captures["s1-mixed"]
    kw = dict(n_streams=1, max_push_bytes=c["cu8"].size, keep_taps=False, crc_repair=1, line_quality=1)
    with wm.Receiver(s1_rescue=1, **kw) as rx:
        rx.push([c["cu8"]])
        lines, recs, reps, quals, levs = rx.lines(), rx.line_rescues(), rx.line_repairs(), rx.line_quality(), rx.line_levels()
        stats = rx.rescue_stats()
    with wm.Receiver(**kw) as rx:
        rx.push([c["cu8"]])
        plain = list(zip(rx.lines(), rx.line_repairs(), rx.line_quality(), rx.line_levels()))
    assert len(lines) == len(recs) == len(reps) == len(quals) == len(levs) and stats == c["want"]["stats"]
    assert [rp for rp in recs] == c["want"]["records"]
    rest = []
    for ln, rec, rep, ql, lv in zip(lines, recs, reps, quals, levs):
        if rec["status"] == 1:
            assert set(rep.values()) == {0} and set(ql.values()) == {0} and lv["n"] > 0 and lv["sync_sample"] < ln["sample"]
        else:
            rest.append((ln, rep, ql, lv))
    assert rest == plain
    # crc_repair may have repaired a line the oracle prints bad: everything else is the restatement's text
    want = c["want"]
    assert [ln["text"] for ln, rec in zip(lines, recs) if rec["status"] == 1] == [t for t, r in zip(want["lines"], want["rescued"]) if r]


def test_batch_sink_in_one_lane(wm, oracle, captures):
    """A batch with both contexts in ONE lane (k3_rescue recorded and issued behind the mate's operations), two passes over the resident
    capture: pass 1 gives the records of the single push, pass 2 those the restatement gives for the second half of the capture fed
    twice -- the same telegrams again, behind a carry."""
    c = captures["s1-l40"]
    cu8, one = c["cu8"], c["want"]
    want2 = RF.rescue_capture(oracle.run(np.concatenate([cu8, cu8]), oracle.make_opts(), taps=True, chips=True), push_m=cu8.size // 4)
    n1 = len(one["lines"])
    assert all(want2[k][:n1] == one[k] for k in ("lines", "crc_ok", "records")) and sum(want2["rescued"][n1:]) >= 3
    got = one_lane(wm, [cu8] * 64, 64, True, push=cu8.size, n_push=2, s1_rescue=1)
    for s in range(64):
        for k, (lo, hi) in enumerate(((0, n1), (n1, None))):
            assert [r["text"] for r in got.lines[s][k]] == want2["lines"][lo:hi]
            assert [r["crc_ok"] for r in got.lines[s][k]] == want2["crc_ok"][lo:hi]
            assert [r["rescue"] for r in got.lines[s][k]] == want2["records"][lo:hi]


def test_batch_sink_reads_the_records(wm, captures):
    """A batch of 64 in two contexts: the sink reads the rescue records of the lines it is handed."""
    c = captures["s1-l40"]
    got = [[] for _ in range(64)]

    def on_push(first, n, recs, timing):
        for r in recs:
            got[r["stream"]].append((dict((k, v) for k, v in r.items() if k not in ("rescue", "level")), r["rescue"]))

    with wm.Batch(64, contexts=2, max_push_bytes=c["cu8"].size, s1_rescue=1) as b:
        for s in range(64):
            b.stage(s, c["cu8"])
        b.run_resident(c["cu8"].size, 1, on_push)
    for s in range(64):
        assert [ln["text"] for ln, _ in got[s]] == c["want"]["lines"] and [rp for _, rp in got[s]] == c["want"]["records"]
        assert [ln["crc_ok"] for ln, _ in got[s]] == c["want"]["crc_ok"]
    p = ctypes.POINTER(wm.Rescue)()
    with wm.Batch(64, contexts=2, max_push_bytes=4096) as b:              # without the field, and outside a sink: 0 / NULL
        assert wm.lib().wmbus_batch_line_rescues(b._h, 0, ctypes.byref(p)) == 0 and not p


def test_cli_and_the_drop_options(wm, captures, tmp_path):
    """-y appends ;y<pairs> to the rescued lines and to no other; with -v the closing count goes to stderr; batch mode prints the same
    behind the file name; only_crc_ok and dedup_twins act behind the rescue."""
    c = captures["s1-l40"]
    cu8, want = c["cu8"], c["want"]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    text = "".join(ln[:-1] + ";y%d\n" % rec["pairs"] if r else ln for ln, rec, r in zip(want["lines"], want["records"], want["rescued"]))
    assert text.count(";y") == want["stats"][1]
    tail = "rescue: %d subjects, %d rescued" % want["stats"]
    one = ["-L", "0", "-B", str(cu8.size)]                  # the capture in one push: which telegrams are subjects depends on the cut
    p = subprocess.run([wm.CLI_PATH, "-v", "-y"] + one, input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == text and p.stderr.decode().splitlines()[-1] == tail
    p = subprocess.run([wm.CLI_PATH, "-v"] + one, input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.decode() == c["ref"]["text"] and b"rescue:" not in p.stderr
    cu8.tofile(tmp_path / "a.cu8")
    p = subprocess.run([wm.CLI_PATH, "-v", "-y", "-B", str(cu8.size), "a.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("a.cu8: " + x + "\n" for x in text.splitlines()) and tail.encode() in p.stderr
    kept, _ = run(wm, cu8, keep_taps=False, only_crc_ok=True)
    assert [ln["text"] for ln, _ in kept] == [ln for ln, ok in zip(want["lines"], want["crc_ok"]) if ok]
    assert [rp for _, rp in kept] == [rp for rp, ok in zip(want["records"], want["crc_ok"]) if ok]
    plain, _ = run(wm, cu8, keep_taps=False, only_crc_ok=True, s1_rescue=0)
    assert len(kept) == len(plain) + want["stats"][1]
    # the run-length framer's line of a rescued telegram is its twin: one of the two is dropped
    twins, _ = run(wm, cu8, keep_taps=False, dedup_twins=True)
    both, _ = run(wm, cu8, keep_taps=False)
    payloads = [ln["text"].split(";0x")[1] for ln, _ in twins]
    assert len(payloads) == len(set(payloads)) and set(payloads) == {ln["text"].split(";0x")[1] for ln, _ in both}



def test_cli_census_counts_a_rescue(wm, oracle, captures):
    """-m with -y: the census has no code of its own for a rescue -- a rescued line is a CRC-clean line with a level record like any
    other, so its burst moves from missed or crc-failed to decoded and CRC-clean, and the transmissions stay what they were.  (The
    census counts the S1 chain only with -s, and finds a burst only over a floor: eight of the capture's telegrams 94 ms apart, rotated
    to where -s looks for S1.)"""
    sigma = RF.SYNTHETIC["s1-l40"][1]
    cu8 = rotated(TR.modulate([("S1", a) for a in captures["s1-l40"]["sent"][:8]], seed=3, amplitude=40, sigma=sigma, gap=150000))
    want = RF.rescue_capture(oracle.run(cu8, oracle.make_opts(simultaneous=1), taps=True, chips=True))
    payload = lambda ln: ln.rstrip().split(";0x")[1]
    clean = {payload(ln) for ln, r, ok in zip(want["lines"], want["rescued"], want["crc_ok"]) if ok and not r}
    seen = {payload(ln) for ln, r in zip(want["lines"], want["rescued"]) if not r}
    new_clean = len({payload(ln) for ln, r in zip(want["lines"], want["rescued"]) if r} - clean)
    new_decoded = len({payload(ln) for ln, r in zip(want["lines"], want["rescued"]) if r} - seen)
    assert new_clean >= 3
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    sums, out = {}, {}
    for sw in ("-m", "-my"):
        p = subprocess.run([wm.CLI_PATH, "-v", "-s", sw, "-L", "0", "-B", str(cu8.size)], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        rows = [ln for ln in p.stderr.decode().splitlines() if ln.endswith("CRC-clean")]
        assert len(rows) == 2, p.stderr[-2000:]               # -s: a row per chain; the S1 chain's is the second
        sums[sw] = [int(x) for x in rows[1].replace(",", "").split() if x.isdigit()][-3:]
        out[sw] = p.stdout.decode()
        print(sw, rows)
    assert out["-m"] == "".join(ln for ln, r in zip(want["lines"], want["rescued"]) if not r)
    (t0, d0, c0), (t1, d1, c1) = sums["-m"], sums["-my"]
    assert t1 == t0 >= 8 and c1 == c0 + new_clean and d1 == d0 + new_decoded and c1 <= d1 <= t1
