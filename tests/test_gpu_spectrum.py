"""cfg.input_spectrum on the GPU: the three arrays of k0_spectrum<fmt, dc> as wmbus_read_spectrum returns them against the numpy restatement
(tests/spectrum_ref.py), bit for bit, over pushes, captures, formats, the DC blocker, the resampler, channels and two input windows; the
reset; a context with the field prints what the context without it prints and stays on the plain path; the CLI's -w; bad arguments."""
import json
import os
import subprocess

import numpy as np
import pytest

import format_ref as FR
import spectrum_ref as PR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS
from test_spectrum_emulated import full_scale_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
BLK = 4096
PUSHES = 3
# Raw bytes per push.  A push is whole 4096-byte units, which hold 4 / 4 / 2 / 1 level blocks of cu8 / cs8 / cs16 / cf32: the small push is
# the smallest one that holds 4 level blocks in every format; the large one is 37 units = 148 / 148 / 74 / 37 level blocks (37 level blocks
# themselves exist in cf32 only), whose runs of 4 level blocks do not fill the last block of four waves, nor -- cs16, cf32 -- the last run.
UNITS = {"4": {FR.CU8: 1, FR.CS8: 1, FR.CS16: 2, FR.CF32: 4}, "37": dict.fromkeys(FORMATS, 37)}

_WANT = {}


def capture(fmt, n_bytes, seed):
    """Random bit patterns (NaN and infinities among the cf32 ones), a different capture per seed."""
    return np.random.default_rng(7700 + 16 * seed + fmt).integers(0, 256, n_bytes, dtype=np.uint8)


def restated(key, raw, fmt, R):
    if key not in _WANT:
        _WANT[key] = PR.spectrum(raw, fmt, R)
    return _WANT[key]


def same(got, want, tag):
    assert got[2] == want[2], tag
    assert np.array_equal(got[1], want[1]), (tag, "peak", int(np.argmax(got[1] != want[1])))
    assert np.array_equal(got[0], want[0]), (tag, "sum", int(np.argmax(got[0] != want[0])))


@pytest.mark.parametrize("R", [0, 6], ids=["R0", "R6"])
@pytest.mark.parametrize("units", ["4", "37"])
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_read_spectrum_equals_the_restatement(wm, fmt, n_streams, units, R):
    """Three pushes; read after every push: the accumulators carry over the pushes of a context and equal the restatement of the stream
    so far.  A different capture per stream, so that a stride mix-up shows."""
    n = UNITS[units][fmt] * BLK
    caps = [capture(fmt, PUSHES * n, s) for s in range(n_streams)]
    with wm.Receiver(n_streams=n_streams, max_push_bytes=n, input_format=fmt, input_dc=R, input_spectrum=1) as rx:
        for k in range(PUSHES):
            rx.push([a[k * n:(k + 1) * n] for a in caps])
            for s in range(n_streams):
                same(rx.read_spectrum(s), restated((fmt, units, R, s, k), caps[s][:(k + 1) * n], fmt, R), (s, k))
        assert rx.resampler_launches() == (PUSHES if R or fmt != FR.CU8 else 0)


def test_behind_a_resampler_with_channels_and_with_two_windows_it_is_the_spectrum_of_the_raw_input(wm):
    """input_rate_hz = 2048000: the survey is of the input, in front of the resampler.  input_channels = 3: one spectrum per capture, the
    arrays of the context without channels.  input_windows = 2: the pushes alternate between the windows."""
    n = 6 * BLK
    for fmt, kw in ((FR.CU8, dict(input_rate_hz=2048000)), (FR.CS16, dict(input_rate_hz=2048000, input_dc=6)),
                    (FR.CS16, dict(input_channel_hz=[700000, -600000, 0], input_rate_hz=4000000)), (FR.CU8, dict(input_channel_hz=[100000, 0, -250000])),
                    (FR.CU8, dict(input_windows=2)), (FR.CF32, dict(input_windows=2, input_dc=6)), (FR.CS8, dict(input_agc=1, input_shift_hz=-120000))):
        caps = [capture(fmt, PUSHES * n, 40 + s) for s in range(2)]
        with wm.Receiver(n_streams=2, max_push_bytes=n, input_format=fmt, input_spectrum=1, **kw) as rx:
            for k in range(PUSHES):
                rx.push([a[k * n:(k + 1) * n] for a in caps])
            for s in range(2):
                same(rx.read_spectrum(s), restated((fmt, "special", kw.get("input_dc", 0), s), caps[s], fmt, kw.get("input_dc", 0)), (fmt, sorted(kw), s))


def test_reset_zeroes_one_capture_and_leaves_the_others(wm):
    n = 2 * BLK
    caps = [capture(FR.CU8, 2 * n, 60 + s) for s in range(3)]
    with wm.Receiver(n_streams=3, max_push_bytes=n, input_spectrum=1) as rx:
        rx.push([a[:n] for a in caps])
        first = [PR.spectrum(a[:n], FR.CU8) for a in caps]
        same(rx.read_spectrum(1, reset=True), first[1], "the read that resets still returns the arrays")
        total, peak, blocks = rx.read_spectrum(1)
        assert blocks == 0 and not total.any() and not peak.any()
        same(rx.read_spectrum(0), first[0], 0)
        same(rx.read_spectrum(2), first[2], 2)
        rx.push([a[n:] for a in caps])
        same(rx.read_spectrum(1), PR.spectrum(caps[1][n:], FR.CU8), "behind the reset: the second push alone")
        same(rx.read_spectrum(0), PR.spectrum(caps[0], FR.CU8), 0)
        same(rx.read_spectrum(2), PR.spectrum(caps[2], FR.CU8), 2)
        # any of the three pointers may be NULL
        L = wm.lib()
        assert L.wmbus_read_spectrum(rx._h, 0, None, None, None, 0) == 512
        p = np.zeros(512, np.uint32)
        assert L.wmbus_read_spectrum(rx._h, 2, None, p.ctypes.data, None, 0) == 512 and np.array_equal(p, PR.spectrum(caps[2], FR.CU8)[1])
        assert L.wmbus_read_spectrum(rx._h, 3, None, None, None, 0) == -1                  # no such capture


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_full_scale_inputs(wm, fmt):
    """The largest pw and the largest z the arithmetic can meet: all samples at the format's negative full scale, and a full-scale tone on
    a bin centre."""
    for name, raw in full_scale_inputs(fmt).items():
        want = PR.spectrum(raw, fmt)
        with wm.Receiver(n_streams=1, max_push_bytes=raw.size, input_format=fmt, input_spectrum=1) as rx:
            rx.push([raw])
            same(rx.read_spectrum(0), want, name)


def test_a_context_with_the_field_prints_what_the_context_without_it_prints(wm, samples):
    """The lines and the level records, on the bundled capture and on a synthetic one; plain cu8 with a survey stays on the plain path;
    the survey of the bundled capture is the restatement's: one transmitter, 10 kHz below the centre."""
    s2 = samples["samples2"][:samples["samples2"].size // BLK * BLK]
    synth = wm.synth_capture(seed=12, n_samples=1 << 19, kinds=15, frames_per_s=60.0)[0]
    for cu8, floor in ((s2, 4), (synth, 5)):
        out = []
        for spectrum in (0, 1):
            with wm.Receiver(n_streams=1, max_push_bytes=1 << 20, line_levels=1, keep_taps=False, input_spectrum=spectrum) as rx:
                text, levels = "", []
                for off in range(0, cu8.size, 1 << 20):
                    text += rx.push([cu8[off:off + (1 << 20)]])
                    levels += rx.line_levels()
                assert rx.resampler_launches() == 0             # the plain path: no conversion kernel
                tm = rx.timing()
                assert tm["input_bytes_out"] == 0 and tm["input_clipped"] == 0
                if spectrum:
                    got = rx.read_spectrum(0)
                    same(got, PR.spectrum(cu8, FR.CU8), "the capture")
                else:
                    with pytest.raises(wm.WmbusError, match="input_spectrum") as e:
                        rx.read_spectrum(0)
                    assert "-1" in str(e.value)                 # WMBUS_EINVAL
            out.append((text, levels))
        assert out[0] == out[1] and len(out[0][0].splitlines()) >= floor and len(out[0][1]) == len(out[0][0].splitlines())
        if cu8 is s2:
            assert out[0][0] == BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
            hits = wm.spectrum_channels(1600000, *got)
            assert hits == PR.channels(1600000, *got) and len(hits) == 1 and abs(hits[0]["offset_hz"] + 10290) <= 3125


def test_in_one_batch_lane(wm, oracle):
    """The stage in a batch lane: two synthetic captures, each in both of two contexts that share ONE lane, four pushes of 2^18 bytes on
    the plain cu8 path -- the survey kernel recorded inside the demodulation kernel's turn and issued behind the mate's operations.  The
    accumulators of every capture after the run equal tests/spectrum_ref.py on the whole capture (in the lane run and in the
    lane-per-context run), the lines are the oracle's."""
    caps = [wm.synth_capture(seed=12 + s, n_samples=1 << 19, kinds=15, frames_per_s=60.0)[0] for s in range(2)]
    want = [oracle.run(c, oracle.make_opts())["text"] for c in caps]
    assert all(len(w.splitlines()) >= 5 for w in want)
    spec = [PR.spectrum(c, FR.CU8) for c in caps]
    assert all(sp[2] == (1 << 19) // PR.N and sp[1].any() for sp in spec)
    seen = []
    got = one_lane(wm, caps + caps, 4, push=1 << 18, n_push=4, input_windows=2, input_spectrum=1,
                   after=lambda b: seen.append([rx.read_spectrum(s) for rx, first, n in b.contexts for s in range(n)]))
    assert got.plan == [(0, 2), (2, 2)] and len(seen) == 2
    for run in seen:
        for s in range(4):
            same(run[s], spec[s % 2], s)
    assert [got.whole_text(s) for s in range(4)] == want + want


def test_cli_survey(wm, samples, tmp_path):
    """rtl_wmbus_hip -w < samples2: the golden's lines on stdout, the single hit and its -O on stderr; with -S also per file in batch mode;
    noise gives none."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    s2 = samples["samples2"]
    whole = s2[:s2.size // BLK * BLK]
    hit = PR.channels(1600000, *PR.spectrum(whole, FR.CU8))
    assert len(hit) == 1
    hz, ratio = hit[0]["offset_hz"], hit[0]["ratio_q8"] / 256.0
    p = subprocess.run([wm.CLI_PATH, "-w", "-v"], input=s2.tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    assert [ln for ln in p.stderr.decode().splitlines() if ln.startswith("spectrum:")] == [f"spectrum: {hz} Hz x{ratio:.1f} over the floor", f"spectrum: -O {hz}"]
    assert p.stdout == subprocess.run([wm.CLI_PATH, "-v"], input=s2.tobytes(), capture_output=True, env=env, timeout=300).stdout
    noise = np.clip(np.rint(127.5 + np.random.default_rng(5).normal(0, 3, 1 << 21)), 0, 255).astype(np.uint8)
    whole.tofile(tmp_path / "a.cu8"); noise.tofile(tmp_path / "b.cu8")
    p = subprocess.run([wm.CLI_PATH, "-w", "-S", "-v", "a.cu8", "b.cu8"], cwd=tmp_path, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    # the shorter file is padded with silence to the longer one's pushes: the survey of a.cu8 is of the bytes the context was given
    err = [ln for ln in p.stderr.decode().splitlines() if "spectrum:" in ln]
    assert err[-1] == "b.cu8: spectrum: nothing above the floor" and err[-2].startswith("a.cu8: spectrum: -O ") and len(err) == 3
    assert abs(int(err[-2].split("-O ")[1]) - hz) <= 3125
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, env=env)
    assert "\t-w " in p.stdout.decode()


def test_bad_arguments_are_refused(wm):
    for bad in (2, 1 << 31):
        with pytest.raises(wm.WmbusError, match="input_spectrum") as e:
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_spectrum=bad)
        assert "(-1)" in str(e.value)                        # WMBUS_EINVAL
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_spectrum=1) as rx:
        rx.stage(0, np.full(BLK, 128, np.uint8))
        rx.process(BLK)
        with pytest.raises(wm.WmbusError, match="collect the push first"):
            rx.read_spectrum(0)
        rx.collect()
        assert rx.read_spectrum(0)[2] == 4
