"""Line quality on the GPU (cfg.line_quality): through the C ABI the quality records equal tests/quality_ref.py on the oracle's taps and
chips and the lines are those of a context without the field -- on the bundled capture under the switches that change how a burst
reaches the burst kernel, cut into pushes, beside crc_repair, line_levels and line_power, behind the drop options, on several streams,
through a batch's sink and the CLI; and a context without the field is the one it was."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import quality_ref as QR
import repair_ref as RR
import telegram_ref as TR
from lanes import one_lane

pytestmark = pytest.mark.gpu

PUSH_M = 1 << 16                                            # the cut of the push test, decimated samples: 4 bytes each
CONFIGS = {"product": dict(keep_taps=False), "one-wave-clock": dict(keep_taps=False, clock_waves=1),
           "systolic-clock": dict(keep_taps=False, clock_waves=4), "rounds-on-host": dict(keep_taps=False, rounds_on_host=True)}


def whole(cu8):
    return np.ascontiguousarray(cu8[:cu8.size // 4096 * 4096])


@pytest.fixture(scope="module")
def bundled(oracle, samples):
    """The bundled 1.6 MS/s capture, the oracle's run of it and the restatement's records: computed once, shared, left unchanged."""
    cu8 = whole(samples["samples2"])
    ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
    return dict(cu8=cu8, ref=ref, lines=ref["text"].splitlines(keepends=True), want=QR.quality_capture(ref), cut=QR.quality_capture(ref, push_m=PUSH_M))


def run(wm, streams, sizes=None, **kw):
    """[(line dict, {name: record of that line})] of the captures `streams` over the pushes `sizes` (bytes; None: one push)."""
    kw.setdefault("line_quality", 1)
    streams = streams if isinstance(streams, list) else [streams]
    sizes = sizes or [streams[0].size]
    out = []
    with wm.Receiver(n_streams=len(streams), max_push_bytes=max(sizes), **kw) as rx:
        off = 0
        for n in sizes:
            rx.push([a[off:off + n] for a in streams]); off += n
            lines = rx.lines()
            recs = dict(quality=rx.line_quality(), repair=rx.line_repairs(), level=rx.line_levels(), power=rx.line_power())
            assert len(recs["quality"]) == (len(lines) if kw["line_quality"] else 0)
            for k, ln in enumerate(lines):
                out.append((ln, {name: r[k] for name, r in recs.items() if r}))
    return out


@pytest.mark.parametrize("config", list(CONFIGS))
def test_against_the_restatement(wm, bundled, config):
    got = run(wm, bundled["cu8"], **CONFIGS[config])
    assert [ln["text"] for ln, _ in got] == bundled["lines"]
    assert [r["quality"] for _, r in got] == bundled["want"]
    assert [r["quality"]["n"] for _, r in got] == [577, 0, 1405, 0] and got[2][1]["quality"]["eye_hz"] < 0 < got[0][1]["quality"]["eye_hz"]


def test_push_cuts(wm, bundled):
    """Eight equal pushes of 2^16 decimated samples: the first time2 telegram straddles 3 x 2^16 and has n = 0, the second lies inside
    the sixth push and has the record of the single push.  The lines are the oracle's either way."""
    want, cut = bundled["want"], bundled["cut"]
    assert [r["n"] > 0 for r in want] == [True, False, True, False] and [r["n"] > 0 for r in cut] == [False, False, True, False]
    total = bundled["cu8"].size
    assert total % (4 * PUSH_M) == 0
    got = run(wm, bundled["cu8"], [4 * PUSH_M] * (total // (4 * PUSH_M)), keep_taps=False)
    assert [ln["text"] for ln, _ in got] == bundled["lines"]
    assert [r["quality"] for _, r in got] == cut
    assert got[2][1]["quality"] == want[2] and got[0][1]["quality"] == QR.ZERO


def test_beside_crc_repair(wm, bundled, oracle):
    """The quality is measured on the chips as received: with crc_repair the records are the same, and the repair's lines and records
    are those of crc_repair alone."""
    both = run(wm, bundled["cu8"], keep_taps=False, crc_repair=1)
    alone = run(wm, bundled["cu8"], keep_taps=False, crc_repair=1, line_quality=0)
    rep = RR.repair_capture(bundled["ref"])
    assert [r["quality"] for _, r in both] == bundled["want"]
    assert [ln["text"] for ln, _ in both] == [ln["text"] for ln, _ in alone] == rep["lines"]
    assert [r["repair"] for _, r in both] == [r["repair"] for _, r in alone] == rep["records"] and sum(rep["repaired"]) == 1
    assert all("quality" not in r for _, r in alone)


def test_beside_levels_and_power(wm, bundled):
    """All three record arrays in step with the lines: each equals the one of a context with that option alone."""
    got = run(wm, bundled["cu8"], keep_taps=False, line_levels=1, line_power=1)
    lev = run(wm, bundled["cu8"], keep_taps=False, line_levels=1, line_quality=0)
    pw = run(wm, bundled["cu8"], keep_taps=False, line_power=1, line_quality=0)
    assert [ln["text"] for ln, _ in got] == bundled["lines"] and len(got) == len(lev) == len(pw)
    assert [r["quality"] for _, r in got] == bundled["want"]
    assert [r["level"] for _, r in got] == [r["level"] for _, r in lev] and all(r["level"]["n"] for _, r in got)
    assert [r["power"] for _, r in got] == [r["power"] for _, r in pw] and all(r["power"]["n_signal"] for _, r in got)


def test_drop_options(wm, bundled):
    """dedup_twins and only_crc_ok act behind the record: a dropped line takes its record along."""
    lines, want = bundled["lines"], bundled["want"]
    ok = run(wm, bundled["cu8"], keep_taps=False, only_crc_ok=True)
    keep = [i for i, ln in enumerate(lines) if ln.split(";")[2] == "1"]
    assert keep == [0, 1]
    assert [ln["text"] for ln, _ in ok] == [lines[i] for i in keep] and [r["quality"] for _, r in ok] == [want[i] for i in keep]
    twins = run(wm, bundled["cu8"], keep_taps=False, dedup_twins=True)
    plain = run(wm, bundled["cu8"], keep_taps=False, dedup_twins=True, line_quality=0)
    assert [ln["text"] for ln, _ in twins] == [ln["text"] for ln, _ in plain] and len(twins) < len(lines)
    assert [r["quality"] for _, r in twins] == [want[lines.index(ln["text"])] for ln, _ in twins]
    assert twins[0][1]["quality"]["n"] == 577


def test_three_streams_s1_and_c1(wm, oracle, bundled):
    """Different captures per stream: six S1 telegrams, six C1 telegrams, and the head of the bundled capture."""
    def air(seed, lfield):
        return TR.frame_a(bytes([lfield]) + bytes(np.random.default_rng(seed).integers(0, 256, lfield).astype(np.uint8)))
    s1 = TR.modulate([("S1", air(50 + i, 12 + 3 * i)) for i in range(6)], seed=7)
    c1 = TR.modulate([("C1A", air(60 + i, 20 + 9 * i)) for i in range(6)], seed=8)
    size = max(s1.size, c1.size)
    size = (size + 4095) // 4096 * 4096
    rng = np.random.default_rng(9)
    caps = [np.concatenate([c, rng.integers(125, 131, size - c.size).astype(np.uint8)]) for c in (s1, c1)] + [bundled["cu8"][:size]]
    assert size <= bundled["cu8"].size
    got = run(wm, caps, keep_taps=False)
    n_meas = []
    for s, cu8 in enumerate(caps):
        ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
        mine = [(ln, r) for ln, r in got if ln["stream"] == s]
        assert [ln["text"] for ln, _ in mine] == ref["text"].splitlines(keepends=True)
        want = QR.quality_capture(ref)
        assert [r["quality"] for _, r in mine] == want
        n_meas.append(sum(r["n"] > 0 for r in want))
    assert n_meas[0] == 6 and n_meas[1] == 6, n_meas
    s1_recs = [r["quality"] for ln, r in got if ln["stream"] == 0 and r["quality"]["n"]]
    assert all(abs(r["chip_rate_chz"] - 3_276_800) < 3_276_800 // 100 for r in s1_recs)      # the modulator's clock is exact; 1 %: a sanity bound, the parity above is the test


def test_batch_sink_in_one_lane(wm, oracle, bundled):
    """The same batch with both contexts in ONE lane (k3_quality recorded and issued behind the mate's operations), two passes over the
    resident capture: pass 1 gives the records of the single push, pass 2 those the restatement gives for the second half of the
    capture fed twice."""
    cu8, one = bundled["cu8"], bundled["want"]
    ref2 = oracle.run(np.concatenate([cu8, cu8]), oracle.make_opts(), taps=True, chips=True)
    lines2, want2, n1 = ref2["text"].splitlines(keepends=True), QR.quality_capture(ref2, push_m=cu8.size // 4), len(one)
    assert lines2[:n1] == bundled["lines"] and want2[:n1] == one and any(r["n"] > 0 for r in one) and any(r["n"] > 0 for r in want2[n1:])
    got = one_lane(wm, [cu8] * 64, 64, True, push=cu8.size, n_push=2, line_quality=1)
    for s in range(64):
        p1, p2 = got.lines[s]
        assert [r["text"] for r in p1] == bundled["lines"] and [r["quality"] for r in p1] == one, s
        assert [r["text"] for r in p2] == lines2[n1:] and [r["quality"] for r in p2] == want2[n1:], s


def test_batch_sink_reads_the_records(wm, bundled):
    """A batch of 64 in two contexts: the sink reads the quality records of the lines it is handed."""
    cu8 = bundled["cu8"]
    got = [[] for _ in range(64)]

    def on_push(first, n, recs, timing):
        for r in recs:
            got[r["stream"]].append((r["text"], r["quality"]))

    with wm.Batch(64, contexts=2, max_push_bytes=cu8.size, line_quality=1) as b:
        for s in range(64):
            b.stage(s, cu8)
        b.run_resident(cu8.size, 1, on_push)
    for s in range(64):
        assert [t for t, _ in got[s]] == bundled["lines"] and [q for _, q in got[s]] == bundled["want"], s
    p = ctypes.POINTER(wm.Quality)()
    with wm.Batch(64, contexts=2, max_push_bytes=4096) as b:              # without the field, and outside a sink: 0 / NULL
        assert wm.lib().wmbus_batch_line_quality(b._h, 0, ctypes.byref(p)) == 0 and not p


def fields(q):
    return f";{q['chip_rate_chz'] // 100}.{q['chip_rate_chz'] % 100:02d};{q['jitter_ns']};{q['eye_hz']}" if q["n"] else ";;;"


def test_cli(wm, bundled, tmp_path):
    """-q appends the three fields to the t2a lines and ;;; to the rla lines; with -v the closing count goes to stderr, in the batch path
    (one push per file: the records of the single push) and in the stream path (the reader cuts the pushes: the fields are those of
    some cut, the summary counts what was printed).  -q -l -n -x: the documented order."""
    cu8, lines, want = bundled["cu8"], bundled["lines"], bundled["want"]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    text = "".join(ln[:-1] + fields(q) + "\n" for ln, q in zip(lines, want))
    assert text.count(";99800.14;1367;32214\n") == 1 and text.count(";99765.30;775;-9951\n") == 1 and text.count(";;;\n") == 2
    cu8.tofile(tmp_path / "a.cu8")
    p = subprocess.run([wm.CLI_PATH, "-v", "-q", "a.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("a.cu8: " + x + "\n" for x in text.splitlines())
    assert "quality: 2 measured, 1 with a closed eye" in p.stderr.decode().splitlines()
    # the stream path
    p = subprocess.run([wm.CLI_PATH, "-v", "-q"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.decode().splitlines(keepends=True)
    print(out, p.stderr.decode().splitlines()[-1])
    assert len(out) == len(lines)
    measured = closed = 0
    for o, ln, q in zip(out, lines, want):
        assert o.startswith(ln[:-1] + ";") and o[len(ln) - 1:] in (fields(q) + "\n", ";;;\n")
        if ln.startswith("rla;"):
            assert o.endswith(";;;\n")
        elif not o.endswith(";;;\n"):
            measured += 1; closed += q["eye_hz"] <= 0
    assert p.stderr.decode().splitlines()[-1] == f"quality: {measured} measured, {closed} with a closed eye"
    p = subprocess.run([wm.CLI_PATH, "-v"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.decode() == bundled["ref"]["text"] and b"quality:" not in p.stderr
    # the order of the fields: -l's, -n's, -x's, -q's
    got = run(wm, cu8, keep_taps=False, line_levels=1, line_power=1, crc_repair=1)
    full = ""
    for ln, r in got:
        lv, pw, rp = r["level"], r["power"], r["repair"]
        full += "a.cu8: " + ln["text"][:-1] + f";{lv['offset_hz']};{lv['dev_hz']};{pw['signal']};{pw['noise']};x{pw['ratio_q8'] / 256.0:.1f}"
        full += (f";x{rp['blocks_repaired']}/{rp['chips_flipped']}" if rp["blocks_bad"] and rp["blocks_repaired"] == rp["blocks_bad"] else "") + fields(r["quality"]) + "\n"
    assert all(r["level"]["n"] and r["power"]["n_signal"] and r["power"]["n_noise"] for _, r in got) and full.count(";x1/1;99765.30;775;-9951\n") == 1
    p = subprocess.run([wm.CLI_PATH, "-v", "-q", "-l", "-n", "-x", "a.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == full


def test_field_off(wm, bundled):
    got = run(wm, bundled["cu8"], keep_taps=False, line_quality=0)
    assert "".join(ln["text"] for ln, _ in got) == bundled["ref"]["text"] and all(not r for _, r in got)
    with open(QR.GOLDEN) as f:
        assert [ln["text"] for ln, _ in got] == json.load(f)["samples2"]["lines"]
    with wm.Receiver(n_streams=1, max_push_bytes=bundled["cu8"].size, keep_taps=False) as rx:
        assert rx.cfg.line_quality == 0
        rx.push([bundled["cu8"]])
        p = ctypes.POINTER(wm.Quality)()
        assert rx.lines_count() == len(got) and wm.lib().wmbus_line_quality(rx._h, ctypes.byref(p)) == 0 and not p
        assert rx.line_levels() == []                       # the field's own switch-on of the level records is not there either
