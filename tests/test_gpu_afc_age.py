"""cfg.input_spectrum_age and cfg.input_channel_afc_hz on the GPU.  The ageing survey: after every push the view (wmbus_read_spectrum), the lock (wmbus_read_input_afc) and the bytes the
pipeline got (wmbus_read_resampled) against the restatement tests/afc_age_ref.py, over formats, the resampler, the DC blocker, the AGC,
two input windows, the plain cu8 path and a reset in mid-stream; a batch; a context without the field; the refusals; the CLI's -E.
The lock per channel: every channel of a list against an independent single-channel AFC context and the restatement; a batch with both
fields; the refusals; the CLI's auto: entries."""
import json
import os
import subprocess

import numpy as np
import pytest

import afc_age_ref as AG
import afc_ref as AF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR
from lanes import one_lane
from test_formats_emulated import design
from test_gpu_afc import GAIN, MIXES, mixed, quantised

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
BLK = 4096
FS = 1600000
PUSH = 8 * BLK                                      # raw bytes per push: 32 / 16 / 8 level blocks of cu8 / cs16 / cf32
PUSHES = 6


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_spectrum_age: on a library without the field no test of this file says anything, so none
    passes."""
    assert "input_spectrum_age" in [f[0] for f in wm.Cfg._fields_]


def three_captures(fmt, fin):
    """Per stream a capture of its own, PUSHES pushes long: a tone of amplitude 0.5 at +25 kHz in pushes 0-1 and one of amplitude 0.1 at
    -20 kHz from push 2 on (the capture of the CPU test: the lock must let go of the first); noise, which never locks; a tone at -30 kHz
    that appears in push 4."""
    n = PUSH // FR.BPS[fmt]
    t = np.arange(PUSHES * n)
    rng = np.random.default_rng(5200 + fmt)
    noise = lambda s: s * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
    tone = lambda f, a, first, last: a * np.exp(2j * np.pi * (f / fin) * t) * ((t >= first * n) & (t < last * n))
    z = [noise(0.004) + tone(25000, 0.5, 0, 2) + tone(-20000, 0.1, 2, PUSHES),
         noise(0.05),
         noise(0.004) + tone(-30000, 0.3, 4, PUSHES)]
    return [quantised(v, fmt) for v in z]


# (format, input rate, input_dc, input_agc, input windows, A, push behind which capture 0 is read with reset or None)
CASES = [(FR.CU8, 0, 0, 0, 1, 3, None), (FR.CU8, 0, 0, 0, 1, 5, None), (FR.CU8, 0, 0, 0, 1, 6, None), (FR.CU8, 0, 0, 0, 1, 6, 2),
         (FR.CS16, 2048000, 6, 1, 1, 5, None), (FR.CF32, 0, 0, 0, 2, 3, None), (FR.CU8, 0, 0, 0, 1, 0, None)]
CASE_IDS = [f"{FR.NAMES[c[0]]}-{c[1] or 'native'}" + (f"-dc{c[2]}" if c[2] else "") + ("-agc" if c[3] else "") + ("-2windows" if c[4] == 2 else "") +
            f"-A{c[5]}" + (f"-reset{c[6]}" if c[6] is not None else "") for c in CASES]


@pytest.mark.parametrize("fmt,rate,R,agc,windows,A,reset_at", CASES, ids=CASE_IDS)
def test_view_state_and_bytes_equal_the_restatement_after_every_push(wm, fmt, rate, R, agc, windows, A, reset_at):
    """Three captures side by side, six pushes of 8 x 4096 raw bytes; after every push read_spectrum, read_input_afc and read_resampled
    of every stream against tests/afc_age_ref.py.  A = 0 on the same input gives today's arrays and today's lock."""
    L, M, taps = design(wm, rate)
    fin = rate or FS
    caps = three_captures(fmt, fin)
    cuts = [PUSH] * PUSHES
    resets = [(reset_at,) if reset_at is not None and s == 0 else () for s in range(3)]
    gain = 0 if agc else 300
    runs = [AG.run(c, fmt, fin, cuts, A, 0, 0, R, agc, gain, L, M, taps, resets=resets[s]) for s, c in enumerate(caps)]
    views = [AG.views(c, fmt, cuts, A, R, resets[s]) for s, c in enumerate(caps)]
    handed = AF.bytes_per_push(runs[0][0], fmt, cuts, L, M)
    states = [[AF.public(p[2]) for p in r[2]] for r in runs]
    # from the restatement alone: what the case is about does occur
    assert all(s["locked"] == 0 for s in states[1])
    if A == 0:
        assert [s["changes"] for s in states[0]] == [1] * PUSHES and runs[0][2] == AF.plans(caps[0], fmt, fin, cuts, 0, 0, R)
    elif fmt == FR.CU8:
        assert states[0][-1]["changes"] == 2 and abs(states[0][-1]["shift_hz"] + 20000) < fin / PR.N / 2
        if reset_at is not None:                                 # A = 6 moves at push 4; with the view emptied behind push 2, at push 3
            assert [s["changes"] for s in states[0]] == [1, 1, 1, 2, 2, 2] and views[0][3][2] == 32
    assert states[2][-1]["locked"] == 1 and states[2][3]["locked"] == 0
    kw = dict(input_format=fmt, input_rate_hz=rate, input_dc=R, input_agc=agc, input_windows=windows, input_afc=1, input_spectrum_age=A)
    if not agc:
        kw["input_gain_q8"] = gain
    with wm.Receiver(n_streams=3, max_push_bytes=PUSH, **kw) as rx:
        off = [0, 0, 0]
        for k in range(PUSHES):
            rx.push([c[k * PUSH:(k + 1) * PUSH] for c in caps])
            for s in range(3):
                assert rx.read_input_afc(s) == states[s][k], (s, k, rx.read_input_afc(s), states[s][k])
                got, want = rx.read_resampled(s), runs[s][0][off[s]:off[s] + handed[k]]
                assert got.size == want.size == handed[k], (s, k)
                assert np.array_equal(got, want), (s, k, int(np.argmax(got != want)))
                off[s] += handed[k]
                total, peak, blocks = rx.read_spectrum(s, reset=k in resets[s])
                assert blocks == views[s][k][2], (s, k, blocks, views[s][k][2])
                assert np.array_equal(peak, views[s][k][1]) and np.array_equal(total, views[s][k][0]), (s, k)
                if A == 0:
                    want_spec = PR.spectrum(caps[s][:(k + 1) * PUSH], fmt, R)
                    assert blocks == want_spec[2] and np.array_equal(peak, want_spec[1]) and np.array_equal(total, want_spec[0])
        assert rx.resampler_launches() == PUSHES


def test_the_plain_cu8_path_stays_plain_with_an_ageing_survey(wm):
    """input_spectrum = 1 with input_spectrum_age = 3 on cu8 at the native rate: no conversion kernel, and the view after every push."""
    cap = three_captures(FR.CU8, FS)[0]
    views = AG.views(cap, FR.CU8, [PUSH] * PUSHES, 3)
    with wm.Receiver(n_streams=1, max_push_bytes=PUSH, input_spectrum=1, input_spectrum_age=3) as rx:
        for k in range(PUSHES):
            rx.push([cap[k * PUSH:(k + 1) * PUSH]])
            total, peak, blocks = rx.read_spectrum(0)
            assert blocks == views[k][2] == 16 and np.array_equal(peak, views[k][1]) and np.array_equal(total, views[k][0]), k
        assert rx.resampler_launches() == 0


def test_batch_with_an_ageing_survey(wm, samples):
    """wmbus_batch over four captures in two contexts, one push each, with input_afc and an epoch longer than the capture (A = 12: 4096
    level blocks): every context carries the age, and every capture's lines are those of its own fixed-shift context at the survey's
    hit, as without the age."""
    caps = [mixed(samples, f) for f in MIXES]
    push = caps[0].size
    assert push // 2 // PR.N <= 1 << 12
    want = []
    for c in caps:
        hz = PR.channels(FS, *PR.spectrum(c, FR.CU8))[0]["offset_hz"]
        with wm.Receiver(n_streams=1, max_push_bytes=push, input_gain_q8=GAIN, input_shift_hz=hz, keep_taps=False) as rx:
            want.append(rx.run(c)[0])
    text = [""] * len(caps)
    with wm.Batch(n_streams=len(caps), contexts=2, max_push_bytes=push, input_windows=2, input_gain_q8=GAIN, input_afc=1, input_spectrum_age=12) as b:
        pos = {}

        def fill(first, n, slab):
            k = push if not pos.get(first) else 0
            for s in range(n):
                slab[s, :k] = caps[first + s][:k]
            pos[first] = 1
            return k

        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        b.run_from(fill, on_push)
        locks = [rx.read_input_afc(s) for rx, first, n in b.contexts for s in range(n)]
        blocks = [rx.read_spectrum(s)[2] for rx, first, n in b.contexts for s in range(n)]
    assert text == want
    assert [a["locked"] for a in locks] == [1] * 4 and len({a["shift_hz"] for a in locks}) == 4
    assert blocks == [push // 2 // PR.N] * 4


def test_batch_in_one_lane_with_an_ageing_survey(wm, oracle, samples):
    """The four captures of the batch test above as two contexts of two in ONE lane, each capture in two pushes of half its length, A = 12:
    the ageing survey (its slot fills recorded too), k0_afc_plan on the view and the AFC form of the input kernel issued behind the mate's
    operations.  Lines against the oracle on tests/afc_age_ref.py's bytes for those two pushes, the locks against its plans, the level
    blocks of the view, and everything against the lane-per-context run."""
    caps = [mixed(samples, f) for f in MIXES]
    cuts = [caps[0].size // 2] * 2
    assert cuts[0] % 4096 == 0 and caps[0].size // 2 // PR.N <= 1 << 12
    want, locks = [], []
    for c in caps:
        y, pl = AG.pipeline_bytes(c, FR.CU8, FS, cuts, 12, g_q8=GAIN)
        want.append(oracle.run(y, oracle.make_opts())["text"]); locks.append(AF.public(pl[-1][2]))
    assert all(len(w.splitlines()) >= 3 for w in want) and len(set(want)) > 1 and len({a["shift_hz"] for a in locks}) == 4
    seen = []
    got = one_lane(wm, caps, 4, push=cuts[0], n_push=2, input_windows=2, input_gain_q8=GAIN, input_afc=1, input_spectrum_age=12,
                   after=lambda b: seen.append([(rx.read_input_afc(s), rx.read_spectrum(s)[2]) for rx, first, n in b.contexts for s in range(n)]))
    assert got.plan == [(0, 2), (2, 2)]
    assert [got.whole_text(s) for s in range(4)] == want
    for run in seen:                                             # the lane run's and the lane-per-context run's
        assert [a for a, _ in run] == locks and [k for _, k in run] == [caps[0].size // 2 // PR.N] * 4


def test_a_context_without_the_field_is_the_context_it_was(wm, samples):
    """Plain cu8 with input_spectrum_age = 0: no conversion kernel, the golden's lines, and no AFC to read."""
    s2 = mixed(samples, 0)
    with wm.Receiver(n_streams=1, max_push_bytes=s2.size, input_spectrum_age=0, keep_taps=False) as rx:
        text = rx.run(s2)[0]
        assert rx.resampler_launches() == 0
        with pytest.raises(wm.WmbusError, match="input_afc"):
            rx.read_input_afc(0)
        with pytest.raises(wm.WmbusError, match="input_spectrum"):
            rx.read_spectrum(0)
    assert text == BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    assert wm._make_cfg(n_streams=1, max_push_bytes=s2.size).input_spectrum_age == 0


def test_bad_arguments_are_refused(wm):
    bad = [dict(input_spectrum_age=5), dict(input_spectrum=1, input_spectrum_age=32), dict(input_afc=1, input_spectrum_age=32),
           dict(input_spectrum_age=1, input_shift_hz=1000)]
    for open_ in (lambda **kw: wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw), lambda **kw: wm.Batch(n_streams=8, max_push_bytes=1 << 16, **kw)):
        for kw in bad:
            with pytest.raises(wm.WmbusError, match="input_spectrum_age") as e:
                open_(**kw)
            assert "(-1)" in str(e.value), str(e.value)      # WMBUS_EINVAL
    for kw in (dict(input_spectrum=1, input_spectrum_age=31), dict(input_afc=1, input_spectrum_age=1)):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw) as rx:
            assert rx.read_spectrum(0)[2] == 0
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_afc=1, input_spectrum_age=2) as rx:
        rx.stage(0, np.full(BLK, 128, np.uint8))
        rx.process(BLK)
        with pytest.raises(wm.WmbusError, match="collect the push first"):
            rx.read_spectrum(0)
        with pytest.raises(wm.WmbusError, match="collect the push first"):
            rx.read_input_afc(0)
        rx.collect()
        assert rx.read_spectrum(0)[2] == 4


def two_halves(samples):
    """The capture of the CPU test: the bundled capture mixed by -43000 Hz, then mixed by +40000 Hz at half the amplitude."""
    s2 = samples["samples2"]
    s2 = s2[:s2.size // (1 << 18) * (1 << 18)]
    x = SR.round_trip_cu8(s2, FS, 40000).astype(np.float64) - 127.5
    return np.concatenate([SR.round_trip_cu8(s2, FS, -43000), np.clip(np.rint(127.5 + 0.5 * x), 0, 255).astype(np.uint8)])


def test_cli_survey_age(wm, samples):
    """rtl_wmbus_hip -E seconds -O auto -v on the two-half capture in pushes of 2^18 bytes, each a fresh process with its own timeout.
    -E 0.1 is A = 9 (2^9 x 512 samples = 0.16 s, the smallest epoch of at least 0.1 s): two afc: lines, the restatement's.  -E 1 is A = 12,
    an epoch of 1.3 s -- as long as the whole capture, so nothing is forgotten yet: one afc: line, as without -E.  Bad spellings, and -E
    without -w or -O auto, are usage errors."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    raw = two_halves(samples)
    cuts = [1 << 18] * (raw.size >> 18)
    assert raw.size // 2 // PR.N <= 1 << 12
    out = {}
    for secs, A in (("0.1", 9), ("1", 12), (None, 0)):
        pl = AG.plans(raw, FR.CU8, FS, cuts, A)
        want, seen = [], 0
        for _, _, st in pl:
            if st["changes"] != seen:
                want.append(f"afc: {st['held_hz']} Hz x{st['ratio_q8'] / 256.0:.1f} over the floor")
                seen = st["changes"]
        args = [wm.CLI_PATH, "-O", "auto", "-v", "-g", "3.22", "-B", str(1 << 18), "-L", "0"] + (["-E", secs] if secs else [])
        p = subprocess.run(args, input=raw.tobytes(), capture_output=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr
        afc = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("afc:")]
        assert afc == want, (secs, afc, want)
        out[A] = (len(afc), len(p.stdout.decode().splitlines()))
    assert out[9][0] == 2 and out[12][0] == 1 and out[0] == out[12] and out[9][1] > out[0][1]
    for bad in (["-E", "0", "-O", "auto"], ["-E", "x", "-O", "auto"], ["-E", "-1", "-w"], ["-E", "1s", "-w"], ["-E", "1"], ["-E", "1", "-O", "25k"]):
        p = subprocess.run([wm.CLI_PATH] + bad, input=b"", capture_output=True, env=env, timeout=120)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-E seconds" in p.stdout.decode(), bad


# ---- a lock per channel (cfg.input_channel_afc_hz) ---------------------------------------------------------------------------------------

import channels_fixture as CF                                              # noqa: E402
from test_afc_age_emulated import CH_HZ, CH_RANGE, WIDE_OFF_HZ, tones_cs16, two_wide_captures     # noqa: E402

GAIN_DB = "4.07"                                     # the CLI's spelling of gain 409 (CF.WIDE_GAIN)


@pytest.fixture()
def the_library_has_the_channel_field(wm):
    assert "input_channel_afc_hz" in [f[0] for f in wm.Cfg._fields_]


def two_narrow_captures():
    """Two cu8 captures at 1.6 MS/s for the list [150000, -150000] with ranges [64000, 0], three pushes of 32 level blocks: capture 0 has
    a transmitter 20 kHz above channel 0 from push 1 on; capture 1 one 30 kHz below channel 0 in every push and a stronger one 25 kHz
    above it in push 2 (the lock moves); both have one 10 kHz beside channel 1, which is fixed and ignores it."""
    n = PUSH // 2
    t = np.arange(3 * n)
    out = []
    for seed, parts in ((71, [(170000, 0.3, n, 3 * n), (-140000, 0.3, 0, 3 * n)]),
                        (72, [(120000, 0.15, 0, 3 * n), (175000, 0.4, 2 * n, 3 * n), (-160000, 0.2, 0, 3 * n)])):
        rng = np.random.default_rng(seed)
        z = 0.004 * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
        for f, a, first, last in parts:
            z = z + a * np.exp(2j * np.pi * (f / FS) * t) * ((t >= first) & (t < last))
        out.append(quantised(z, FR.CU8))
    return out, [PUSH] * 3


CHANNEL_CASES = {"cs16-4M": (FR.CS16, CF.WIDE_FS, CH_HZ, CH_RANGE), "cu8-native-two": (FR.CU8, 0, [150000, -150000], [64000, 0])}


@pytest.mark.parametrize("case", list(CHANNEL_CASES))
def test_every_channel_is_its_own_afc_context(wm, case, the_library_has_the_channel_field):
    """Two captures, a channel list with a range per channel, three pushes.  For every pipeline stream v = capture x C + channel the
    lock and read_resampled after every push equal those of an independent single-channel context with input_shift_hz = hz[c],
    input_afc = 1, input_afc_range_hz = range[c] fed the same pushes -- the existing feature as the oracle -- and the restatement; a
    fixed channel (range 0) reads {hz[c], 0, 0, 0} and its bytes are those of the channels context without the array."""
    fmt, rate, hz, ranges = CHANNEL_CASES[case]
    fin = rate or FS
    L, M, taps = design(wm, rate)
    caps, cuts = two_wide_captures() if fmt == FR.CS16 else two_narrow_captures()
    C = len(hz)
    gain = 300
    want = [AG.channel_plans(c, fmt, fin, cuts, hz, ranges) for c in caps]                     # [capture][channel][push]
    # from the restatement alone: a lock that moves occurs, and on the wideband list a following channel that never locks
    assert any(want[k][c][-1][2]["changes"] == 2 for k in range(2) for c in range(C))
    assert fmt != FR.CS16 or any(want[k][c][-1][2]["locked"] == 0 for k in range(2) for c in range(C) if ranges[c])
    kw = dict(n_streams=2, max_push_bytes=cuts[0], input_format=fmt, input_rate_hz=rate, input_gain_q8=gain)
    got_state, got_bytes = {}, {}
    with wm.Receiver(input_channel_hz=hz, input_channel_afc_hz=ranges, **kw) as rx:
        for v in range(2 * C):
            assert rx.read_input_afc(v) == dict(shift_hz=hz[v % C], locked=0, changes=0, ratio_q8=0)
        for i, n in enumerate(cuts):
            rx.push([c[i * n:(i + 1) * n] for c in caps])
            for v in range(2 * C):
                got_state[v, i], got_bytes[v, i] = rx.read_input_afc(v), rx.read_resampled(v).copy()
        assert rx.resampler_launches() == len(cuts)
        with pytest.raises(wm.WmbusError):
            rx.read_input_afc(2 * C)
        total, peak, blocks = rx.read_spectrum(1)                # the survey is on by itself, per capture
        spec = PR.spectrum(caps[1], fmt)
        assert blocks == spec[2] and np.array_equal(peak, spec[1]) and np.array_equal(total, spec[0])
    for c in range(C):
        if ranges[c]:
            ctx = wm.Receiver(input_shift_hz=hz[c], input_afc=1, input_afc_range_hz=ranges[c], **kw)
        else:
            ctx = wm.Receiver(input_channel_hz=hz, **kw)
        with ctx as rx:
            off = [0, 0]
            for i, n in enumerate(cuts):
                rx.push([a[i * n:(i + 1) * n] for a in caps])
                for k in range(2):
                    v = k * C + c
                    step, base, st = want[k][c][i]
                    assert got_state[v, i] == AF.public(st), (v, i)
                    if ranges[c]:
                        assert rx.read_input_afc(k) == got_state[v, i], (v, i)
                        single = rx.read_resampled(k)
                    else:
                        assert got_state[v, i] == dict(shift_hz=hz[c], locked=0, changes=0, ratio_q8=0)
                        single = rx.read_resampled(v)
                    assert np.array_equal(got_bytes[v, i], single), (v, i)
    for k in range(2):                                           # and the restated bytes of every stream
        for c in range(C):
            y, _ = AF.convert(caps[k], fmt, cuts, [(p[0], p[1]) for p in want[k][c]], 0, 0, gain, L, M, taps)
            have = np.concatenate([got_bytes[k * C + c, i] for i in range(len(cuts))])
            assert np.array_equal(have, y[:have.size]) and have.size == y.size // BLK * BLK, (k, c)


def test_batch_with_channel_afc_and_an_ageing_survey(wm, samples, the_library_has_the_channel_field):
    """wmbus_batch over four captures in two contexts, one push each -- the bundled capture mixed by -43000, +60000, -30000 and as it is --
    with the list [-40000, 50000], ranges of 32000 and A = 12: the lines of channel c of every capture are those of a single-channel
    context with input_shift_hz = hz[c], input_afc = 1, input_afc_range_hz = 32000 and the same age on that capture."""
    caps = [mixed(samples, f) for f in MIXES]
    push = caps[0].size
    hz, ranges = [-40000, 50000], [32000, 32000]
    want, locks_want = {}, {}
    for c, f in enumerate(hz):
        with wm.Receiver(n_streams=len(caps), max_push_bytes=push, input_gain_q8=GAIN, input_shift_hz=f, input_afc=1, input_afc_range_hz=ranges[c],
                         input_spectrum_age=12, keep_taps=False) as rx:
            for k, text in enumerate(rx.run(caps)):
                want[k, c] = text
                locks_want[k, c] = rx.read_input_afc(k)
    assert sum(len(t.splitlines()) for t in want.values()) >= 12 and sum(a["locked"] for a in locks_want.values()) == 4
    text = {key: "" for key in want}
    with wm.Batch(n_streams=len(caps), contexts=2, max_push_bytes=push, input_windows=2, input_gain_q8=GAIN, input_channel_hz=hz, input_channel_afc_hz=ranges,
                  input_spectrum_age=12) as b:
        pos = {}

        def fill(first, n, slab):
            k = push if not pos.get(first) else 0
            for s in range(n):
                slab[s, :k] = caps[first + s][:k]
            pos[first] = 1
            return k

        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"], ln["channel"]] += ln["text"]
        b.run_from(fill, on_push)
        locks = {(first + s, c): rx.read_input_afc(s * 2 + c) for rx, first, n in b.contexts for s in range(n) for c in range(2)}
    assert text == want and locks == locks_want


def test_batch_in_one_lane_with_channel_afc_and_an_ageing_survey(wm, samples, the_library_has_the_channel_field):
    """The batch above with its two contexts in ONE lane and every capture in two pushes of half its length: the lines and the locks of
    channel c of every capture are those of the single-channel context on that capture in the same two pushes."""
    caps = [mixed(samples, f) for f in MIXES]
    half = caps[0].size // 2
    hz, ranges = [-40000, 50000], [32000, 32000]
    want, locks_want = {}, {}
    for c, f in enumerate(hz):
        with wm.Receiver(n_streams=len(caps), max_push_bytes=half, input_gain_q8=GAIN, input_shift_hz=f, input_afc=1, input_afc_range_hz=ranges[c],
                         input_spectrum_age=12, keep_taps=False) as rx:
            for k, text in enumerate(rx.run(caps, push_bytes=half)):
                want[k, c] = text
                locks_want[k, c] = rx.read_input_afc(k)
    assert sum(len(t.splitlines()) for t in want.values()) >= 12 and sum(a["locked"] for a in locks_want.values()) == 4
    seen = []
    got = one_lane(wm, caps, 4, push=half, n_push=2, input_windows=2, input_gain_q8=GAIN, input_channel_hz=hz, input_channel_afc_hz=ranges, input_spectrum_age=12,
                   after=lambda b: seen.append({(first + s, c): rx.read_input_afc(s * 2 + c) for rx, first, n in b.contexts for s in range(n) for c in range(2)}))
    assert got.plan == [(0, 2), (2, 2)]
    text = {(k, c): "".join(ln["text"] for push in got.lines[k] for ln in push if ln["channel"] == c) for k in range(4) for c in range(2)}
    assert text == want and seen == [locks_want, locks_want]


def test_bad_channel_afc_arguments_are_refused(wm, the_library_has_the_channel_field):
    bad = [dict(input_channel_afc_hz=[64000]),                                                        # without channels
           dict(input_channel_hz=[100000, -100000], input_channel_afc_hz=[0, 0, 5000]),              # an entry beyond the list
           dict(input_channel_hz=[700000, -100000], input_channel_afc_hz=[100001, 0]),               # |hz| + range beyond Fin / 2
           dict(input_channel_hz=[-799000, 0], input_channel_afc_hz=[1001, 0]),
           dict(input_channel_hz=[100000, -100000], input_channel_afc_hz=[64000, 0], input_afc=1),   # together with input_afc
           dict(input_channel_afc_hz=[64000], input_afc=1)]
    for open_ in (lambda **kw: wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw), lambda **kw: wm.Batch(n_streams=8, max_push_bytes=1 << 16, **kw)):
        for kw in bad:
            with pytest.raises(wm.WmbusError, match="input_channel_afc_hz|input_afc together with input_channels") as e:
                open_(**kw)
            assert "(-1)" in str(e.value), str(e.value)      # WMBUS_EINVAL
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_channel_hz=[700000, -799000], input_channel_afc_hz=[100000, 1000]) as rx:
        assert rx.read_input_afc(1) == dict(shift_hz=-799000, locked=0, changes=0, ratio_q8=0)
        rx.stage(0, np.full(BLK, 128, np.uint8))
        rx.process(BLK)
        with pytest.raises(wm.WmbusError, match="collect the push first"):
            rx.read_input_afc(1)
        rx.collect()
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_channel_hz=[100000, -100000]) as rx:     # all ranges 0: no AFC to read
        with pytest.raises(wm.WmbusError, match="input_afc"):
            rx.read_input_afc(0)


def test_cli_channel_list_with_auto_entries(wm, the_library_has_the_channel_field):
    """rtl_wmbus_hip -O auto:700k,auto:-600k,0 -R 4M -I cs16 -v on the wideband capture whose transmitters sit at 730000, -625000 and 0 Hz,
    a fresh process with its own timeout: stderr has an afc[<channel Hz>]: line per following channel, at the restatement's lock, and
    stdout is that of a run with the locks as a fixed list (the channel field of a line is the list's entry).  The bad spellings."""
    raw = CF.wideband(wm, hz=WIDE_OFF_HZ)[0]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    base = [wm.CLI_PATH, "-R", "4M", "-I", "cs16", "-g", GAIN_DB, "-v", "-B", str(raw.size), "-L", "0"]
    pl = AG.channel_plans(raw, FR.CS16, CF.WIDE_FS, [raw.size], CF.WIDE_HZ[:2], [64000] * 2)
    locks = [pl[c][0][2] for c in range(2)]
    p = subprocess.run(base + ["-O", "auto:700k,auto:-600k,0"], input=raw.tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    afc = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("afc")]
    assert afc == [f"afc[{f}]: {st['held_hz']} Hz x{st['ratio_q8'] / 256.0:.1f} over the floor" for f, st in zip(CF.WIDE_HZ[:2], locks)], p.stderr
    q = subprocess.run(base + ["-O", f"{locks[0]['held_hz']},{locks[1]['held_hz']},0"], input=raw.tobytes(), capture_output=True, env=env, timeout=300)
    assert q.returncode == 0, q.stderr
    strip = lambda out: [ln.rsplit(";", 1)[0] for ln in out.decode().splitlines()]
    chans = lambda out: [ln.rsplit(";", 1)[1] for ln in out.decode().splitlines()]
    assert strip(p.stdout) == strip(q.stdout) and len(strip(p.stdout)) >= 20
    assert set(chans(p.stdout)) == {"700000", "-600000", "0"} and [c == "0" for c in chans(p.stdout)] == [c == "0" for c in chans(q.stdout)]
    for bad in ("auto,325k", "325k,auto", "auto:,5k", "auto:x,5k", "5k,auto:", "auto:325k,auto"):
        p = subprocess.run([wm.CLI_PATH, "-O", bad], input=b"", capture_output=True, env=env, timeout=120)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "auto:Hz" in p.stdout.decode(), bad
