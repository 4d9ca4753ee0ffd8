"""Line levels on the GPU (cfg.line_levels): every record equals tests/level_ref.py on the oracle's soft symbols at the record's own
access-code sample, that sample is a sync-flag chip of the oracle's chip stream, the records do not depend on how the input is cut into
pushes, and the lines are the ones a context without the option prints."""
import ctypes
import os
import subprocess

import pytest

import numpy as np

import level_ref as LR
from lanes import one_lane

pytestmark = pytest.mark.gpu

# pushes in bytes: uneven, one of a single block, one long
CUTS = [4096 * 7, 4096 * 20, 4096, 4096 * 64]
# The longest telegram of a chain in decimated samples (800 kS/s): the most chips a decoder takes after an access code (290 bytes of 12
# chips at 100 kchip/s, of 16 chips at 32.768 kchip/s; wm_dev.h WM_MAXCHIPS_*) at the nominal chip rate, and 1024 samples for a
# transmitter's clock tolerance (the figure wm_decoder.c's twin filter allows).
LONGEST = {0: (12 * 290 + 1) * 8 + 1024, 1: int((16 * 290 + 1) * 800 / 32.768) + 1024}


def cut_sizes(total, cuts=CUTS):
    """`total` bytes as the pushes CUTS, repeated until the capture ends (whole 4096-byte blocks)."""
    out, left, k = [], total // 4096 * 4096, 0
    while left:
        n = min(cuts[k % len(cuts)], left)
        out.append(n); left -= n; k += 1
    return out


def run_levels(wm, caps, sizes, **kw):
    """Per capture: [(line dict, level dict)] over all pushes, in line order."""
    kw.setdefault("line_levels", 1)
    per = [[] for _ in caps]
    with wm.Receiver(n_streams=len(caps), max_push_bytes=max(sizes), **kw) as rx:
        off = 0
        for n in sizes:
            rx.push([c[off:off + n] for c in caps]); off += n
            lines, levels = rx.lines(), rx.line_levels()
            assert len(levels) == (len(lines) if kw["line_levels"] else 0)
            for k, ln in enumerate(lines):
                per[ln["stream"]].append((ln, levels[k] if levels else None))
            tim = rx.timing()
    return per, tim


def check_against_oracle(records, ref):
    """Every record of one capture against the oracle's taps and chips; the line text against the oracle's."""
    assert "".join(ln["text"] for ln, _ in records) == ref["text"]
    sync = {(ch, al): set(LR.sync_chips(ref["chips"], ch, al).tolist()) for ch in (0, 1) for al in (0, 1)}
    valid = 0
    for ln, lv in records:
        ch = ln["chain"]
        assert lv == LR.level(ref["dphi_fir"][ch], lv["sync_sample"], ch), (ln, lv)
        assert lv["sync_sample"] in sync[(ch, ln["algo"])], (ln, lv)
        assert lv["sync_sample"] <= ln["sample"] and ln["sample"] - lv["sync_sample"] <= LONGEST[ch], (ln, lv)
        valid += lv["n"] != 0
    return valid


def oracle_of(oracle, cu8, **opts):
    return oracle.run(cu8[:cu8.size // 4096 * 4096], oracle.make_opts(**opts), taps=True, chips=True)


@pytest.fixture(scope="module")
def parity(wm, oracle):
    """The parity capture (2^20 samples at 1.6 MS/s, every kind, 150 frames/s), the oracle's taps, chips and text of it, and the
    records of one push of it: computed once, shared, left unchanged."""
    cu8, _ = wm.synth_capture(seed=0x1E7E1, n_samples=1 << 20, kinds=wm.T1 | wm.C1A | wm.C1B | wm.S1, frames_per_s=150.0)
    ref = oracle_of(oracle, cu8)
    (one,), tim = run_levels(wm, [cu8], [cu8.size], keep_taps=False)
    return dict(cu8=cu8, ref=ref, one=one, tim=tim)


def test_parity_one_push_and_cut(wm, parity):
    """Case 1.  In one push (as the CLI opens a context: RSSI on demand) and cut into uneven pushes (with debug views: the other burst path)."""
    cu8, ref, one = parity["cu8"], parity["ref"], parity["one"]
    (cut,), _ = run_levels(wm, [cu8], cut_sizes(cu8.size))
    assert [lv for _, lv in one] == [lv for _, lv in cut]
    assert [(ln["text"], ln["sample"]) for ln, _ in one] == [(ln["text"], ln["sample"]) for ln, _ in cut]
    assert len(one) == len(ref["text"].splitlines()) >= 60
    assert check_against_oracle(one, ref) >= len(one) - 4          # all but telegrams at the very start of the stream are measured
    check_against_oracle(cut, ref)
    (plain,), _ = run_levels(wm, [cu8], [cu8.size], keep_taps=False, line_levels=0)
    assert [ln for ln, _ in plain] == [ln for ln, _ in one]
    # what the figures mean.  The mean absolute deviation of an alternating preamble lies between a sine's, 2 / pi of the peak (a C1
    # preamble of +-45 kHz behind the low-pass: 28.6 kHz, 10 % off for noise and the window's ends: 25 kHz) and a square wave's, the
    # peak itself (50 kHz); the generator draws the carrier within +-10 kHz, a quarter on top for the measurement itself.
    clean = [lv for ln, lv in one if ln["crc_ok"] and lv["n"]]
    odd = [lv for lv in clean if not 25000 <= lv["dev_hz"] <= 50000 or abs(lv["offset_hz"]) > 12500]
    assert len(clean) >= 50 and not odd, odd[:5]


SWITCHES = {
    "issue48-d3-s-o": dict(decimation=3, simultaneous=True, remove_dc=True),
    "synth-d5-s": dict(decimation=5, simultaneous=True),
    "synth-d16-4096": dict(decimation=16),
    "rounds-on-host": dict(rounds_on_host=True),
    "bursts-to-host": dict(bursts_to_host=True),
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_other_switches(wm, oracle, samples, parity, name):
    """Case 2: the same checks, one push against cut pushes, under other switches."""
    kw = SWITCHES[name]
    d, s = kw.get("decimation", 2), kw.get("simultaneous", False)
    cuts = CUTS
    if name.startswith("issue48"):
        cu8 = samples["issue48"]
    elif name.startswith("synth"):
        centre = 325.0 if s else 0.0
        cu8, _ = wm.synth_capture(seed=0x5EED + d, n_samples=1 << 20, fs_khz=800 * d, kinds=15, frames_per_s=150.0 if d < 16 else 400.0, t1c1_center_khz=centre, s1_center_khz=-centre)
        if d == 16:
            cuts = [4096]                                         # 128 decimated samples a push: shorter than the carried tail
    else:
        cu8 = parity["cu8"]
    ref = parity["ref"] if cu8 is parity["cu8"] else oracle_of(oracle, cu8, decimation=d, simultaneous=int(s), remove_dc=int(kw.get("remove_dc", False)))
    total = cu8.size // 4096 * 4096
    (one,), _ = run_levels(wm, [cu8], [total], keep_taps=False, **kw)
    (cut,), _ = run_levels(wm, [cu8], cut_sizes(total, cuts), keep_taps=False, **kw)
    assert [lv for _, lv in one] == [lv for _, lv in cut] and [ln for ln, _ in one] == [ln for ln, _ in cut]
    assert len(one) >= 2 and check_against_oracle(one, ref) >= 1          # (the bundled capture holds one telegram, printed by both framers)
    (plain,), _ = run_levels(wm, [cu8], [total], keep_taps=False, line_levels=0, **kw)
    assert [ln for ln, _ in plain] == [ln for ln, _ in one]
    if not name.startswith("synth") and not name.startswith("issue48"):
        assert [lv for _, lv in one] == [lv for _, lv in parity["one"]]          # the other path to a line gives the same records


@pytest.fixture(scope="module")
def eight(wm, oracle):
    caps = [wm.synth_capture(seed=0xE16 + i, n_samples=1 << 18, kinds=15, frames_per_s=200.0)[0] for i in range(8)]
    return caps, [oracle_of(oracle, c) for c in caps]


def test_several_captures_two_input_windows(wm, eight):
    """Case 3a: eight captures in one context with two input windows, cut into pushes."""
    caps, refs = eight
    per, _ = run_levels(wm, caps, cut_sizes(caps[0].size), keep_taps=False, input_windows=2)
    for records, ref in zip(per, refs):
        assert len(records) >= 10
        check_against_oracle(records, ref)


def test_batch_sink_collects_levels(wm, eight):
    """Case 3b: a Batch of 64 in two contexts; the sink reads the levels of the lines it is handed."""
    caps, refs = eight
    got = [[] for _ in range(64)]
    firsts = set()

    def on_push(first, n, recs, timing):
        firsts.add(first)
        for r in recs:
            assert first <= r["stream"] < first + n
            got[r["stream"]].append((r, r["level"]))

    with wm.Batch(64, contexts=2, max_push_bytes=caps[0].size, line_levels=1) as b:
        for s in range(64):
            b.stage(s, caps[s % 8])
        st = b.run_resident(caps[0].size, 1, on_push)
    assert firsts == {0, 32} and st["lines"] == sum(len(g) for g in got)
    for s in range(64):
        assert len(got[s]) >= 10
        check_against_oracle(got[s], refs[s % 8])


def test_batch_sink_in_one_lane(wm, oracle, eight):
    """Case 3b with both contexts in ONE lane (k3_levels and k3_level_tail recorded and issued behind the mate's operations) and two
    passes over the resident captures: every record of both passes against the oracle's taps and chips of the capture fed twice -- the
    second pass's telegrams at the start of the push read the carried tail."""
    caps, _ = eight
    refs2 = [oracle_of(oracle, np.concatenate([c, c])) for c in caps]
    got = one_lane(wm, [caps[s % 8] for s in range(64)], 64, True, push=caps[0].size, n_push=2, line_levels=1)
    assert got.plan == [(0, 32), (32, 32)]
    for s in range(64):
        p1, p2 = got.lines[s]
        assert len(p1) >= 10 and len(p2) >= 10
        assert check_against_oracle([(r, r["level"]) for r in p1 + p2], refs2[s % 8]) >= 20


@pytest.mark.parametrize("opts", [dict(dedup_twins=True), dict(dedup_twins=True, only_crc_ok=True)], ids=["dedup-twins", "only-crc-ok"])
def test_dropped_lines_take_their_levels_along(wm, parity, opts):
    """dedup_twins / only_crc_ok drop a level with its line: the lines that stay keep the records they have in the plain run, in one
    push and cut into pushes (run_levels checks a level per line after every push)."""
    cu8, one = parity["cu8"], parity["one"]
    key = lambda ln: (ln["sample"], ln["chain"], ln["algo"], ln["text"])
    plain = {key(ln): lv for ln, lv in one}
    assert len(plain) == len(one)
    for sizes in ([cu8.size], cut_sizes(cu8.size)):
        (kept,), _ = run_levels(wm, [cu8], sizes, keep_taps=False, **opts)
        assert 20 <= len(kept) < len(one)                          # every clean telegram is printed by both framers: about half the lines go
        assert all(plain[key(ln)] == lv for ln, lv in kept)
        if "only_crc_ok" in opts:
            assert all(ln["crc_ok"] for ln, _ in kept)


def test_cli_switch(wm, parity, tmp_path):
    """Case 4: -l appends ;offset_hz;dev_hz (empty where nothing was measured) in live and in batch mode; without it the output is the
    reference's, byte for byte."""
    cu8, ref, one = parity["cu8"], parity["ref"], parity["one"]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    want = "".join(ln["text"][:-1] + (f";{lv['offset_hz']};{lv['dev_hz']}\n" if lv["n"] else ";;\n") for ln, lv in one)
    p = subprocess.run([wm.CLI_PATH, "-v", "-l"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == want
    p = subprocess.run([wm.CLI_PATH, "-v"], input=cu8.tobytes(), capture_output=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.decode() == ref["text"]
    cu8.tofile(tmp_path / "a.cu8")
    p = subprocess.run([wm.CLI_PATH, "-v", "-l", "a.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.decode() == "".join("a.cu8: " + x + "\n" for x in want.splitlines())
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, env=env, timeout=60)
    assert p.stdout.decode().count("\t-l append ;offset_hz;dev_hz") == 1


def test_default_context_has_no_levels(wm, parity):
    """Case 5: a context opened without the field returns 0 records and a NULL array, and its wmbus_timing is the struct it was: the
    level kernels are no stage of their own (they run inside gather_ms where they run at all)."""
    cu8 = parity["cu8"]
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, keep_taps=False) as rx:
        assert rx.cfg.line_levels == 0
        rx.push([cu8])
        assert rx.lines_count() >= 60 and rx.line_levels() == []
        p = ctypes.POINTER(wm.Level)()
        assert wm.lib().wmbus_line_levels(rx._h, ctypes.byref(p)) == 0 and not p
        tim = rx.timing()
    assert sorted(tim) == sorted(parity["tim"]) and ctypes.sizeof(wm.Timing) == 152      # the struct of the parent commit
    assert all(tim[k] > 0 for k in ("demod_ms", "clock_ms", "rla_ms", "gather_ms"))
    with pytest.raises(wm.WmbusError):
        wm.Receiver(n_streams=1, line_levels=2)
