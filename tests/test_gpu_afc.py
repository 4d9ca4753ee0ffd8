"""cfg.input_afc on the GPU: after every push the lock (wmbus_read_input_afc) and the bytes the pipeline got (wmbus_read_resampled) against
the restatement tests/afc_ref.py, over formats, the resampler, the DC blocker, the AGC, two input windows and a nominal off zero; the
equivalence with a fixed shift on the bundled capture; a batch of captures each locked to its own offset; a context without the field;
the refusals; the CLI's -O auto."""
import json
import os
import subprocess

import numpy as np
import pytest

import afc_ref as AF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS, design

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
BLK = 4096
FS = 1600000
PUSH = 8 * BLK                                      # raw bytes per push: 32 / 32 / 16 / 8 level blocks of cu8 / cs8 / cs16 / cf32
PUSHES = 3
GAIN = SR.CU8_ROUND_TRIP_GAIN
MIXES = [-43000, 60000, -30000, 0]                  # Hz the bundled capture is mixed by, one capture of the batch each


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_afc: on a library without the field no test of this file says anything, so none passes."""
    assert "input_afc" in [f[0] for f in wm.Cfg._fields_] and "wmbus_read_input_afc" in wm.EXPORTS and hasattr(wm.lib(), "wmbus_read_input_afc")


def quantised(z, fmt):
    """Complex samples of magnitude <= 1 as raw bytes of the format."""
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    if fmt == FR.CU8:
        return FR.raw_bytes(np.clip(np.rint(127.5 + 127.0 * v), 0, 255).astype(np.uint8), fmt)
    if fmt == FR.CS8:
        return FR.raw_bytes(np.clip(np.rint(127.0 * v), -128, 127).astype(np.int8), fmt)
    if fmt == FR.CS16:
        return FR.raw_bytes(np.clip(np.rint(32000.0 * v), -32768, 32767).astype(np.int16), fmt)
    return FR.raw_bytes(v.astype(np.float32), fmt)


def three_captures(fmt, fin, nominal):
    """Per stream a capture of its own, PUSHES pushes long: noise, which never locks; a tone 25 kHz above the nominal that first appears
    in push 1; a weak tone 40 kHz below the nominal in push 0 and a ten times stronger one 30 kHz above that -- more than two bins
    away -- in push 2: lock, hold and change all occur."""
    n = PUSH // FR.BPS[fmt]
    t = np.arange(PUSHES * n)
    rng = np.random.default_rng(4100 + fmt)
    noise = lambda s: s * (rng.normal(size=t.size) + 1j * rng.normal(size=t.size))
    tone = lambda f, a, first, last: a * np.exp(2j * np.pi * (f / fin) * t) * ((t >= first * n) & (t < last * n))
    z = [noise(0.05),
         noise(0.004) + tone(nominal + 25000, 0.5, 1, PUSHES),
         noise(0.004) + tone(nominal - 40000, 0.05, 0, PUSHES) + tone(nominal - 10000, 0.5, 2, PUSHES)]
    return [quantised(v, fmt) for v in z]


_WANT = {}


def restated(wm, fmt, rate, nominal, R, agc):
    """(captures, per capture (bytes, clipped, plans), bytes handed on per push), computed once per case."""
    key = (fmt, rate, nominal, R, agc)
    if key not in _WANT:
        L, M, taps = design(wm, rate)
        fin = rate or FS
        caps = three_captures(fmt, fin, nominal)
        cuts = [PUSH] * PUSHES
        runs = [AF.run(c, fmt, fin, cuts, nominal, 0, R, agc, 0 if agc else 300, L, M, taps) for c in caps]
        _WANT[key] = (caps, runs, AF.bytes_per_push(runs[0][0], fmt, cuts, L, M))
    return _WANT[key]


CASES = [(fmt, rate, 0, 0, 0, 1) for fmt in FORMATS for rate in (0, 2048000)] + [
    (FR.CS16, 0, 0, 6, 0, 1), (FR.CU8, 2048000, 0, 0, 1, 1), (FR.CU8, 0, 0, 0, 0, 2), (FR.CS8, 0, -20000, 0, 0, 1), (FR.CF32, 2048000, 30000, 6, 1, 2)]
CASE_IDS = [f"{FR.NAMES[c[0]]}-{c[1] or 'native'}" + (f"-nominal{c[2]}" if c[2] else "") + (f"-dc{c[3]}" if c[3] else "") + ("-agc" if c[4] else "") +
            ("-2windows" if c[5] == 2 else "") for c in CASES]


@pytest.mark.parametrize("fmt,rate,nominal,R,agc,windows", CASES, ids=CASE_IDS)
def test_state_and_bytes_equal_the_restatement_after_every_push(wm, fmt, rate, nominal, R, agc, windows):
    """Three captures side by side, three pushes of 8 x 4096 raw bytes; after every push read_input_afc and read_resampled of every
    stream against tests/afc_ref.py, and the survey (which input_afc switches on by itself) of one of them."""
    caps, runs, handed = restated(wm, fmt, rate, nominal, R, agc)
    states = [[AF.public(p[2]) for p in r[2]] for r in runs]
    # from the restatement alone: the sequence of states the test is about does occur
    assert [s["locked"] for s in states[0]] == [0, 0, 0] and all(s["shift_hz"] == nominal for s in states[0])
    assert [s["locked"] for s in states[1]] == [0, 1, 1] and [s["changes"] for s in states[1]] == [0, 1, 1]
    assert [s["changes"] for s in states[2]] == [1, 1, 2] and abs(states[2][2]["shift_hz"] - states[2][1]["shift_hz"]) > AF.hysteresis(rate or FS)
    assert abs(states[1][2]["shift_hz"] - (nominal + 25000)) < 4000 and abs(states[2][0]["shift_hz"] - (nominal - 40000)) < 4000
    kw = dict(input_format=fmt, input_rate_hz=rate, input_shift_hz=nominal, input_dc=R, input_agc=agc, input_windows=windows, input_afc=1)
    if not agc:
        kw["input_gain_q8"] = 300
    with wm.Receiver(n_streams=3, max_push_bytes=PUSH, **kw) as rx:
        for s in range(3):
            assert rx.read_input_afc(s) == dict(shift_hz=nominal, locked=0, changes=0, ratio_q8=0)
        off = [0, 0, 0]
        for k in range(PUSHES):
            rx.push([c[k * PUSH:(k + 1) * PUSH] for c in caps])
            for s in range(3):
                assert rx.read_input_afc(s) == states[s][k], (s, k)
                got, want = rx.read_resampled(s), runs[s][0][off[s]:off[s] + handed[k]]
                assert got.size == want.size == handed[k], (s, k)
                assert np.array_equal(got, want), (s, k, int(np.argmax(got != want)))
                off[s] += handed[k]
            # the survey is on by itself: the accumulators of the stream so far
            total, peak, blocks = rx.read_spectrum(2)
            want_spec = PR.spectrum(caps[2][:(k + 1) * PUSH], fmt, R)
            assert blocks == want_spec[2] and np.array_equal(peak, want_spec[1]) and np.array_equal(total, want_spec[0])
        assert rx.resampler_launches() == PUSHES


def mixed(samples, f):
    s2 = samples["samples2"]
    s2 = s2[:s2.size // BLK * BLK]
    return SR.round_trip_cu8(s2, FS, f) if f else s2


def test_one_push_is_the_context_with_the_fixed_shift(wm, oracle, samples):
    """The bundled capture mixed by -43000 as one push: the lock is the survey's hit; lines, level records and resampled bytes equal those
    of a context with input_shift_hz = the reported shift_hz, and the lines are the oracle's on the restated bytes -- the four lines of
    the CPU test."""
    raw = mixed(samples, -43000)
    hit = PR.channels(FS, *PR.spectrum(raw, FR.CU8))[0]
    out = []
    for kw in (dict(input_afc=1), None):
        if kw is None:
            kw = dict(input_shift_hz=out[0][3]["shift_hz"], input_spectrum=1)
        with wm.Receiver(n_streams=1, max_push_bytes=raw.size, input_gain_q8=GAIN, line_levels=1, **kw) as rx:
            text = rx.push([raw])
            out.append((text, rx.line_levels(), rx.read_resampled(0).copy(), rx.read_input_afc(0) if "input_afc" in kw else None, rx.timing()["input_clipped"]))
    assert out[0][3] == dict(shift_hz=hit["offset_hz"], locked=1, changes=1, ratio_q8=hit["ratio_q8"]) and hit["offset_hz"] == -53674
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2]) and out[0][4] == out[1][4]
    want = oracle.run(SR.pipeline_bytes(raw, FR.CU8, FS, hit["offset_hz"], GAIN), oracle.make_opts())["text"]
    assert out[0][0] == want and len(want.splitlines()) == 4 and sum(ln.split(";")[2] == "1" for ln in want.splitlines()) >= 3


def test_batch_locks_every_capture_to_its_own_offset(wm, samples):
    """wmbus_batch over four captures -- the bundled capture mixed by -43000, +60000, -30000 and as it is -- in one push each: every
    capture's lines are those of its own fixed-shift context at the survey's hit.  No single input_shift_hz does that."""
    caps = [mixed(samples, f) for f in MIXES]
    push = caps[0].size
    want = []
    for c in caps:
        hz = PR.channels(FS, *PR.spectrum(c, FR.CU8))[0]["offset_hz"]
        with wm.Receiver(n_streams=1, max_push_bytes=push, input_gain_q8=GAIN, input_shift_hz=hz, keep_taps=False) as rx:
            want.append(rx.run(c)[0])
    assert all(len(w.splitlines()) >= 3 for w in want) and len(set(want)) > 1
    text = [""] * len(caps)
    with wm.Batch(n_streams=len(caps), contexts=2, max_push_bytes=push, input_windows=2, input_gain_q8=GAIN, input_afc=1) as b:
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
    assert text == want
    assert [a["locked"] for a in locks] == [1] * 4 and len({a["shift_hz"] for a in locks}) == 4


def test_batch_in_one_lane_locks_every_capture_to_its_own_offset(wm, oracle, samples):
    """The four captures of the batch test above as two contexts of two in ONE lane, each capture in two pushes of half its length: the
    survey, k0_afc_plan and the AFC form of the input kernel recorded and issued behind the mate's operations, the second push behind a
    carried lock.  Lines against the oracle on tests/afc_ref.py's bytes for those two pushes, the locks against its plans, everything
    against the lane-per-context run."""
    caps = [mixed(samples, f) for f in MIXES]
    cuts = [caps[0].size // 2] * 2
    assert cuts[0] % BLK == 0
    want, locks = [], []
    for c in caps:
        y, pl = AF.pipeline_bytes(c, FR.CU8, FS, cuts, g_q8=GAIN)
        want.append(oracle.run(y, oracle.make_opts())["text"]); locks.append(AF.public(pl[-1][2]))
    assert all(len(w.splitlines()) >= 3 for w in want) and len(set(want)) > 1 and len({a["shift_hz"] for a in locks}) == 4
    seen = []
    got = one_lane(wm, caps, 4, push=cuts[0], n_push=2, input_windows=2, input_gain_q8=GAIN, input_afc=1,
                   after=lambda b: seen.append([rx.read_input_afc(s) for rx, first, n in b.contexts for s in range(n)]))
    assert got.plan == [(0, 2), (2, 2)]
    assert [got.whole_text(s) for s in range(4)] == want
    assert seen[0] == locks and seen[1] == locks                 # the lane run's and the lane-per-context run's


def test_a_context_without_the_field_is_the_context_it_was(wm, samples):
    """Plain cu8 without input_afc: no conversion kernel, the golden's lines, and no AFC to read."""
    s2 = mixed(samples, 0)
    with wm.Receiver(n_streams=1, max_push_bytes=s2.size, input_afc=0, keep_taps=False) as rx:
        text = rx.run(s2)[0]
        assert rx.resampler_launches() == 0
        with pytest.raises(wm.WmbusError, match="input_afc") as e:
            rx.read_input_afc(0)
        assert "-1" in str(e.value)                          # WMBUS_EINVAL
    assert text == BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    cfg = wm._make_cfg(n_streams=1, max_push_bytes=s2.size, keep_taps=False)
    assert cfg.input_afc == 0 and cfg.input_afc_range_hz == 0


def test_bad_arguments_are_refused(wm):
    bad = [dict(input_afc=2), dict(input_afc=1, input_channel_hz=[325000, -325000]), dict(input_afc=1, input_afc_range_hz=800001),
           dict(input_afc=1, input_shift_hz=750000), dict(input_afc=1, input_shift_hz=-400000, input_afc_range_hz=400001),
           dict(input_afc=1, input_rate_hz=2048000, input_afc_range_hz=1024001), dict(input_afc_range_hz=1000)]
    for open_ in (lambda **kw: wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw), lambda **kw: wm.Batch(n_streams=8, max_push_bytes=1 << 16, **kw)):
        for kw in bad:
            with pytest.raises(wm.WmbusError, match="input_afc") as e:
                open_(**kw)
            assert "(-1)" in str(e.value), str(e.value)      # WMBUS_EINVAL
    for kw in (dict(input_afc=1, input_afc_range_hz=800000), dict(input_afc=1, input_shift_hz=-400000, input_afc_range_hz=400000),
               dict(input_afc=1, input_rate_hz=2048000, input_shift_hz=960000)):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw) as rx:
            assert rx.read_input_afc(0)["locked"] == 0
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_afc=1) as rx:
        silence = np.full(BLK, 128, np.uint8)               # x = 1 in cu8: a little DC, which the rule reports as a transmitter at 0 Hz
        rx.stage(0, silence)
        rx.process(BLK)
        with pytest.raises(wm.WmbusError, match="collect the push first"):
            rx.read_input_afc(0)
        rx.collect()
        want = AF.public(AF.plans(silence, FR.CU8, FS, [BLK])[0][2])
        assert rx.read_input_afc(0) == want and want["shift_hz"] == 0 and want["locked"] == 1
        assert wm.lib().wmbus_read_input_afc(rx._h, 1, None) == -1 and wm.lib().wmbus_read_input_afc(rx._h, 0, None) == -1


def test_cli_auto_offset(wm, oracle, samples, tmp_path):
    """rtl_wmbus_hip -O auto -v on the -43000 mix, a fresh process with its own timeout: the lines of a run with the lock as -O, and one
    afc: line on stderr per change of the lock.  -O auto:200k on the +200000 mix does the same around its nominal.  -O auto with a list
    is a usage error."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for f, opt in ((-43000, "auto"), (200000, "auto:200k")):
        raw = mixed(samples, f)
        p = subprocess.run([wm.CLI_PATH, "-O", opt, "-v", "-g", "3.22", "-B", str(raw.size)], input=raw.tobytes(), capture_output=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr
        hit = PR.channels(FS, *PR.spectrum(raw, FR.CU8))[0]
        afc = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("afc:")]
        assert afc == [f"afc: {hit['offset_hz']} Hz x{hit['ratio_q8'] / 256.0:.1f} over the floor"], p.stderr
        q = subprocess.run([wm.CLI_PATH, "-O", str(hit["offset_hz"]), "-v", "-g", "3.22", "-B", str(raw.size)], input=raw.tobytes(), capture_output=True, env=env,
                           timeout=120)
        assert q.returncode == 0 and p.stdout == q.stdout and len(p.stdout.decode().splitlines()) == 4
    for bad in ("auto,325k", "325k,auto", "auto:", "auto:x", "automatic"):
        p = subprocess.run([wm.CLI_PATH, "-O", bad], input=b"", capture_output=True, env=env, timeout=120)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-O auto" in p.stdout.decode(), bad
    a, b = mixed(samples, -43000), mixed(samples, 60000)
    a.tofile(tmp_path / "a.cu8"); b.tofile(tmp_path / "b.cu8")
    p = subprocess.run([wm.CLI_PATH, "-O", "auto", "-v", "-g", "3.22", "-B", str(a.size), "a.cu8", "b.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    afc = sorted(ln for ln in p.stderr.decode().splitlines() if "afc:" in ln)
    assert len(afc) == 2 and afc[0].startswith("a.cu8: afc: -53674 Hz") and afc[1].startswith("b.cu8: afc: 49434 Hz")
    out = p.stdout.decode().splitlines()
    assert sum(ln.startswith("a.cu8: ") for ln in out) == 4 and sum(ln.startswith("b.cu8: ") for ln in out) == 4
