"""CRC repair on the GPU (cfg.crc_repair): through the C ABI the lines, wmbus_line.crc_ok and the repair records equal the oracle's text
plus tests/repair_ref.py on the oracle's taps and chips -- on the three captures the header names, under the switches that change how a
burst reaches the burst kernel, cut into pushes, beside -s and a channel list, through a batch's sink and the CLI; and a context
without the field is the one it was."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import channels_fixture as CF
import format_ref as FR
import repair_ref as RR
from lanes import one_lane

pytestmark = pytest.mark.gpu

PUSH_SAMPLES = 1 << 16                                      # the cut of the push test, input samples
CONFIGS = {"product": dict(keep_taps=False), "debug-views": dict(keep_taps=True), "one-wave-clock": dict(keep_taps=False, clock_waves=1),
           "systolic-clock": dict(keep_taps=False, clock_waves=4), "rounds-on-host": dict(keep_taps=False, rounds_on_host=True)}


def whole(cu8):
    return np.ascontiguousarray(cu8[:cu8.size // 4096 * 4096])


@pytest.fixture(scope="module")
def captures(oracle, samples):
    """The three captures, the oracle's run of each and what the restatement makes of it: computed once, shared, left unchanged."""
    caps = {"samples2": whole(samples["samples2"])}
    sent = {}
    for name, (mode, sigma) in RR.SYNTHETIC.items():
        caps[name], sent[name] = RR.synthetic(mode, sigma)
    out = {}
    for name, cu8 in caps.items():
        ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
        out[name] = dict(cu8=cu8, ref=ref, want=RR.repair_capture(ref), cut=RR.repair_capture(ref, push_m=PUSH_SAMPLES // 2), sent=sent.get(name))
    return out


def run(wm, cu8, sizes=None, **kw):
    """[(line dict, repair dict or None)] of one capture over the pushes `sizes` (bytes; None: one push)."""
    kw.setdefault("crc_repair", 1)
    sizes = sizes or [cu8.size]
    out = []
    with wm.Receiver(n_streams=1, max_push_bytes=max(sizes), **kw) as rx:
        off = 0
        for n in sizes:
            rx.push([cu8[off:off + n]]); off += n
            lines, reps = rx.lines(), rx.line_repairs()
            assert len(reps) == (len(lines) if kw["crc_repair"] else 0)
            out += [(ln, reps[k] if reps else None) for k, ln in enumerate(lines)]
    return out


def check(got, want):
    """Byte for byte: the text, crc_ok, the records."""
    assert [ln["text"] for ln, _ in got] == want["lines"]
    assert [ln["crc_ok"] for ln, _ in got] == want["crc_ok"]
    assert [rp for _, rp in got] == want["records"]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["samples2"] + list(RR.SYNTHETIC))
def test_against_the_restatement(wm, captures, name, config):
    c = captures[name]
    got = run(wm, c["cu8"], **CONFIGS[config])
    check(got, c["want"])
    assert sum(c["want"]["repaired"]) >= 1
    if name == "samples2":
        assert got[2][1] == dict(blocks_bad=1, blocks_repaired=1, chips_flipped=1, weight=got[2][1]["weight"]) and got[2][0]["text"].startswith("t2a;T1;1;1;")
    else:                                                   # no false repair: a repaired line carries a telegram that was sent
        sent = {RR.TR.printed_hex(False, a, len(a)) for a in c["sent"]}
        for (ln, rp), rep in zip(got, c["want"]["repaired"]):
            if rep:
                assert ln["text"].rstrip().split(";0x")[1] in sent


@pytest.mark.parametrize("name", ["samples2"] + list(RR.SYNTHETIC))
def test_push_cuts(wm, captures, name):
    """Pushes of 2^16 samples: a subject inside a push is repaired as in the single push, a telegram that straddles a push edge is
    finished by the host decoders and keeps the oracle's line."""
    c = captures[name]
    total = c["cu8"].size
    sizes = [min(2 * PUSH_SAMPLES, total - off) for off in range(0, total, 2 * PUSH_SAMPLES)]
    got = run(wm, c["cu8"], sizes, keep_taps=False)
    check(got, c["cut"])
    one, cut, plain = c["want"], c["cut"], c["ref"]["text"].splitlines(keepends=True)
    for i, (ln, rp) in enumerate(got):
        if cut["repaired"][i]:
            assert one["repaired"][i] and ln["text"] == one["lines"][i] and rp == one["records"][i]
        elif one["repaired"][i]:                            # repaired in one push, cut by an edge here
            assert ln["text"] == plain[i] and rp == RR.ZERO
    print(name, "repaired in one push", sum(one["repaired"]), "cut into pushes", sum(cut["repaired"]))


def test_the_cut_does_cost_a_repair_somewhere(captures):
    """The push test meets a telegram that is repaired in one push and straddles an edge of the 2^16-sample pushes."""
    assert any(sum(c["cut"]["repaired"]) < sum(c["want"]["repaired"]) for c in captures.values())


@pytest.mark.parametrize("name", ["samples2"] + list(RR.SYNTHETIC))
def test_field_off(wm, captures, name):
    c = captures[name]
    got = run(wm, c["cu8"], keep_taps=False, crc_repair=0)
    assert "".join(ln["text"] for ln, _ in got) == c["ref"]["text"]
    with wm.Receiver(n_streams=1, max_push_bytes=c["cu8"].size, keep_taps=False) as rx:
        assert rx.cfg.crc_repair == 0
        rx.push([c["cu8"]])
        p = ctypes.POINTER(wm.Repair)()
        assert rx.lines_count() == len(got) and wm.lib().wmbus_line_repairs(rx._h, ctypes.byref(p)) == 0 and not p
        assert rx.line_levels() == []                       # the field's own switch-on of the level records is not there either


def test_beside_simultaneous(wm, oracle, samples):
    """-s on the bundled 2.4 MS/s capture: the lines of crc_repair = 0 except for what the restatement repairs (there may be nothing)."""
    cu8 = whole(samples["issue48"])
    kw = dict(decimation=3, simultaneous=True, keep_taps=False)
    ref = oracle.run(cu8, oracle.make_opts(decimation=3, simultaneous=1), taps=True, chips=True)
    want = RR.repair_capture(ref)
    check(run(wm, cu8, **kw), want)
    off = run(wm, cu8, crc_repair=0, **kw)
    assert "".join(ln["text"] for ln, _ in off) == ref["text"]
    assert [a != b for a, b in zip(want["lines"], ref["text"].splitlines(keepends=True))] == want["repaired"]
    print("issue48 -s: subjects", want["subjects"], "repaired", sum(want["repaired"]))


def test_beside_a_channel_list(wm, oracle):
    """Two channels of the wideband fixture in one context: every channel's lines and records are the restatement's on the bytes the
    pipeline got for that channel."""
    raw = CF.wideband(wm)[0]
    hz = CF.WIDE_HZ[:2]
    kw = dict(n_streams=1, max_push_bytes=raw.size, input_rate_hz=CF.WIDE_FS, input_format=FR.CS16, input_gain_q8=CF.WIDE_GAIN, input_channel_hz=hz)
    with wm.Receiver(crc_repair=1, **kw) as rx:
        rx.push([raw])
        lines, reps = rx.lines(), rx.line_repairs()
        bytes_ = [rx.read_resampled(v) for v in range(2)]
    with wm.Receiver(**kw) as rx:
        rx.push([raw])
        plain = rx.lines()
    assert len(lines) == len(reps) == len(plain) >= 12
    n_sub = 0
    for c in range(2):
        ref = oracle.run(whole(bytes_[c]), oracle.make_opts(), taps=True, chips=True)
        want = RR.repair_capture(ref)
        check([(ln, rp) for ln, rp in zip(lines, reps) if ln["channel"] == c], want)
        assert "".join(ln["text"] for ln in plain if ln["channel"] == c) == ref["text"]
        n_sub += want["subjects"]
    print("two channels: subjects", n_sub)


def test_batch_sink_in_one_lane(wm, oracle, captures):
    """The same batch with both contexts in ONE lane (k3_repair recorded and issued behind the mate's operations), two passes over the
    resident capture: pass 1 gives the records of the single push, pass 2 those the restatement gives for the second half of the
    capture fed twice -- the same telegrams again, behind a carry."""
    c = captures["samples2"]
    cu8, one = c["cu8"], c["want"]
    want2 = RR.repair_capture(oracle.run(np.concatenate([cu8, cu8]), oracle.make_opts(), taps=True, chips=True), push_m=cu8.size // 4)
    n1 = len(one["lines"])
    assert all(want2[k][:n1] == one[k] for k in ("lines", "crc_ok", "records")) and sum(one["repaired"]) >= 1 and sum(want2["repaired"][n1:]) >= 1
    got = one_lane(wm, [cu8] * 64, 64, True, push=cu8.size, n_push=2, crc_repair=1)
    split = lambda push: [(dict((k, v) for k, v in r.items() if k != "repair"), r["repair"]) for r in push]
    for s in range(64):
        check(split(got.lines[s][0]), one)
        check(split(got.lines[s][1]), {k: want2[k][n1:] for k in ("lines", "crc_ok", "records")})


def test_batch_sink_reads_the_records(wm, captures):
    """A batch of 64 in two contexts: the sink reads the repair records of the lines it is handed."""
    c = captures["samples2"]
    got = [[] for _ in range(64)]

    def on_push(first, n, recs, timing):
        for r in recs:
            got[r["stream"]].append((dict((k, v) for k, v in r.items() if k != "repair"), r["repair"]))

    with wm.Batch(64, contexts=2, max_push_bytes=c["cu8"].size, crc_repair=1) as b:
        for s in range(64):
            b.stage(s, c["cu8"])
        b.run_resident(c["cu8"].size, 1, on_push)
    for s in range(64):
        check(got[s], c["want"])
    p = ctypes.POINTER(wm.Repair)()
    with wm.Batch(64, contexts=2, max_push_bytes=4096) as b:              # without the field, and outside a sink: 0 / NULL
        assert wm.lib().wmbus_batch_line_repairs(b._h, 0, ctypes.byref(p)) == 0 and not p


def test_cli_and_the_drop_options(wm, captures, tmp_path):
    """-x appends ;x1/1 to the one repaired line of the bundled capture; with -v the closing count goes to stderr; only_crc_ok, acting
    behind the repair, keeps the line."""
    c = captures["samples2"]
    cu8, want = c["cu8"], c["want"]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    text = "".join(ln[:-1] + ";x1/1\n" if rep else ln for ln, rep in zip(want["lines"], want["repaired"]))
    assert text.count(";x1/1\n") == 1
    p = subprocess.run([wm.CLI_PATH, "-v", "-x"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == text and p.stderr.decode().splitlines()[-1] == "repair: 1 subjects, 1 repaired"
    p = subprocess.run([wm.CLI_PATH, "-v"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.decode() == c["ref"]["text"] and b"repair:" not in p.stderr
    cu8.tofile(tmp_path / "a.cu8")
    p = subprocess.run([wm.CLI_PATH, "-v", "-x", "a.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("a.cu8: " + x + "\n" for x in text.splitlines()) and b"repair: 1 subjects, 1 repaired" in p.stderr
    kept = run(wm, cu8, keep_taps=False, only_crc_ok=True)
    assert [ln["text"] for ln, _ in kept] == [ln for ln, ok in zip(want["lines"], want["crc_ok"]) if ok] and len(kept) == 3
    assert [rp for _, rp in kept] == [rp for rp, ok in zip(want["records"], want["crc_ok"]) if ok]
    assert len(run(wm, cu8, keep_taps=False, only_crc_ok=True, crc_repair=0)) == 2
