"""cfg.input_agc on the GPU: the bytes, the clip count, the byte count and the gain table of k0_agc_gain -> the AG instantiations of the
two K0-stage kernels against the numpy restatement (tests/agc_ref.py), without and with the DC blocker in front; weak cs16 captures at
2.048 MS/s through a single context, a batch and the CLI (-g auto) print the oracle's text on the restated bytes, and nothing at gain
x 1; input_agc = 0 is the context it always was; bad arguments."""
import os
import subprocess

import numpy as np
import pytest

import agc_ref as AR
import format_ref as FR
from lanes import one_lane
from test_agc_emulated import KINDS, jump_input, x_of
from test_dc_emulated import OUT_HZ, dc_inputs
from test_formats_emulated import FMT_IDS, FORMATS
from test_resample_emulated import BLK, CUTS, N_BLOCKS

pytestmark = pytest.mark.gpu

RATES = [0, 2048000]
SHIFT = 250000


def design(wm, rate):
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, OUT_HZ)
    return L, M, taps


_WANT = {}


def restated(wm, key, raw, fmt, R, fin, f, rate):
    """agc_ref.convert of one capture, computed once per (input, format, R, rate, shift) and shared by the cuts and windows."""
    k = key + (fmt, R, rate, f)
    if k not in _WANT:
        L, M, taps = design(wm, rate)
        _WANT[k] = AR.convert(raw, fmt, R, fin, f, L, M, taps)
    return _WANT[k]


@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven", "each-4096"])
@pytest.mark.parametrize("n_streams", [1, 8])
@pytest.mark.parametrize("R", [0, 6], ids=["R0", "R6"])
@pytest.mark.parametrize("rate", RATES, ids=["native", "2048000"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_bytes_clip_count_and_gain_equal_the_restatement(wm, fmt, rate, R, n_streams, cut, windows):
    """A different capture per stream (the jump input of the emulated test first, then the blocker's named inputs, then random bit
    patterns), so that a stride or a table mix-up shows; the 250 kHz shift behind the blocker on the cs16 and cu8 cases with R = 6."""
    fin = rate or OUT_HZ
    f = SHIFT if R and fmt in (FR.CS16, FR.CU8) else 0
    named = dict(jump=jump_input(fmt, N_BLOCKS * BLK), **dc_inputs(fmt, N_BLOCKS * BLK))
    rng = np.random.default_rng(3000 * fmt + n_streams)
    names = list(named)
    caps = [named[names[s]] if s < len(names) else rng.integers(0, 256, N_BLOCKS * BLK, dtype=np.uint8) for s in range(n_streams)]
    keys = [(names[s],) if s < len(names) else ("random", n_streams, s) for s in range(n_streams)]
    with wm.Receiver(n_streams=n_streams, max_push_bytes=N_BLOCKS * BLK, input_rate_hz=rate, input_shift_hz=f, input_format=fmt, input_dc=R,
                     input_agc=1, input_windows=windows) as rx:
        got, gains, off, clipped, bytes_out = [[] for _ in caps], [[] for _ in caps], 0, 0, 0
        for n in CUTS[cut]:
            rx.push([a[off:off + n] for a in caps]); off += n
            for s in range(n_streams):
                got[s].append(rx.read_resampled(s))
                g = rx.read_input_gain(s)
                assert g.shape == (n // FR.BPS[fmt] // AR.BLOCK,)
                gains[s].append(g.astype(np.int64))
            tm = rx.timing()
            clipped += tm["input_clipped"]; bytes_out += tm["input_bytes_out"]
        assert rx.resampler_launches() == len(CUTS[cut])
    want_clips = 0
    for s in range(n_streams):
        y, clips, g = restated(wm, keys[s], caps[s], fmt, R, fin, f, rate)
        want = y[:y.size // BLK * BLK]
        have, have_g = np.concatenate(got[s]), np.concatenate(gains[s])
        assert np.array_equal(have_g, g), (s, int(np.argmax(have_g != g)))
        assert have.size == want.size, s
        assert np.array_equal(have, want), (s, int(np.argmax(have != want)))
        want_clips += clips
    assert clipped == want_clips
    assert bytes_out == n_streams * restated(wm, keys[0], caps[0], fmt, R, fin, f, rate)[0].size


_WEAK = {}


def weak_captures(wm, oracle):
    """The three weak cs16 captures and the oracle's text on tests/agc_ref.py's bytes of each: computed once, shared, left unchanged."""
    if not _WEAK:
        L, M, T, taps = wm.resampler_design(2048000, OUT_HZ)
        cu8s = [wm.synth_capture(seed=8400 + s, n_samples=1 << 20, fs_khz=2048, kinds=KINDS, frames_per_s=60.0, amplitude=20.0, noise_sigma=3.0)[0] for s in range(3)]
        caps = [FR.raw_bytes(4 * x_of(c), FR.CS16) for c in cu8s]
        want = [oracle.run(AR.pipeline_bytes(c, FR.CS16, 0, 2048000, 0, L, M, taps), oracle.make_opts())["text"] for c in caps]
        assert all(len(w.splitlines()) >= 10 for w in want)
        for c in caps:
            c.setflags(write=False)
        _WEAK.update(caps=caps, want=want)
    return _WEAK["caps"], _WEAK["want"]


def test_weak_cs16_captures_in_one_lane(wm, oracle):
    """The batch of the test below as two contexts of two captures in ONE lane (the fourth capture is the first again), four pushes of
    2^20 bytes: k0_agc_gain and the AGC form of the input kernel recorded and issued behind the mate's operations."""
    caps, want = weak_captures(wm, oracle)
    got = one_lane(wm, caps + [caps[0]], 4, push=1 << 20, n_push=caps[0].size >> 20, input_windows=2, input_rate_hz=2048000, input_format=FR.CS16, input_agc=1)
    assert got.plan == [(0, 2), (2, 2)] and caps[0].size >> 20 == 4
    assert [got.whole_text(s) for s in range(4)] == want + [want[0]]


def test_weak_cs16_captures_give_the_oracles_text_on_the_restated_bytes(wm, oracle, tmp_path):
    """Three 2.048 MS/s synthetic captures (amplitude 20 cu8 steps, noise sigma 3) written as cs16 = 4 (2u - 255), a 160-count amplitude:
    a single context in one push and in odd pushes, a batch and the CLI (-I cs16 -R 2.048M -g auto -v; on stdin, and in batch mode with a
    shorter file padded with silence) print what the oracle prints on tests/agc_ref.py's bytes.  At gain x 1 nothing is received."""
    L, M, T, taps = wm.resampler_design(2048000, OUT_HZ)
    caps, want = weak_captures(wm, oracle)
    opts = oracle.make_opts()
    kw = dict(input_rate_hz=2048000, input_format=FR.CS16)
    with wm.Receiver(n_streams=3, max_push_bytes=caps[0].size, **kw) as rx:      # gain x 1
        assert rx.run(caps) == ["", "", ""]
    kw["input_agc"] = 1
    with wm.Receiver(n_streams=3, max_push_bytes=caps[0].size, **kw) as rx:
        assert rx.run(caps) == want
        g = rx.read_input_gain(0)
        assert g.shape == ((1 << 20) // AR.BLOCK,) and g.min() >= 96 * 65536 // (4 * 2 * 255)      # |x| <= 4 x 255 per component
    with wm.Receiver(n_streams=3, max_push_bytes=1 << 20, input_windows=2, keep_taps=False, **kw) as rx:
        assert rx.run(caps, push_bytes=BLK * 97) == want
        assert rx.read_input_gain(2).shape[0] > 0            # the level's feedback needs no debug views
    push = 1 << 20
    text = [""] * 3
    with wm.Batch(n_streams=3, max_push_bytes=push, input_windows=2, **kw) as b:
        pos = {}

        def fill(first, n, slab):
            off = pos.get(first, 0)
            k = min(push, caps[0].size - off)
            for s in range(n):
                slab[s, :k] = caps[first + s][off:off + k]
            pos[first] = off + k
            return k

        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        st = b.run_from(fill, on_push)
        assert st["samples"] == 3 * caps[0].size // 4
    assert text == want
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    cli = [wm.CLI_PATH, "-I", "cs16", "-R", "2.048M", "-g", "auto", "-v", "-B", str(1 << 20)]
    p = subprocess.run(cli, input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == want[0]
    # batch mode: the shorter file is padded with the format's silence (0: P = 0, the gain at its clamp, the constant byte 128)
    caps[0].tofile(tmp_path / "a.cs16"); caps[1][:3 << 20].tofile(tmp_path / "b.cs16")
    pad = np.concatenate([caps[1][:3 << 20], np.zeros(caps[0].size - (3 << 20), np.uint8)])
    want_b = oracle.run(AR.pipeline_bytes(pad, FR.CS16, 0, 2048000, 0, L, M, taps), opts)["text"]
    p = subprocess.run(cli + ["a.cs16", "b.cs16"], cwd=tmp_path, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    got = {"a.cs16": "", "b.cs16": ""}
    for line in p.stdout.decode().splitlines(True):
        name, rest = line.split(": ", 1)
        got[name] += rest
    assert got == {"a.cs16": want[0], "b.cs16": want_b}


def test_agc_zero_is_the_plain_path_and_agc_alone_is_a_stage(wm, oracle):
    cu8 = wm.synth_capture(seed=12, n_samples=1 << 18, kinds=KINDS, frames_per_s=60.0)[0]
    want = oracle.run(cu8, oracle.make_opts())["text"]
    assert len(want.splitlines()) >= 5
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_agc=0) as rx:
        assert rx.run(cu8)[0] == want
        assert rx.resampler_launches() == 0
        tm = rx.timing()
        assert tm["input_clipped"] == 0 and tm["input_bytes_out"] == 0
        with pytest.raises(wm.WmbusError, match="input_agc"):
            rx.read_input_gain(0)
        with pytest.raises(wm.WmbusError):
            rx.read_resampled(0)
    # a context that converts without the AGC has no gains to read either
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_format=wm.FMT_CS8, input_dc=6) as rx:
        rx.push([FR.embed(cu8, FR.CS8)])
        with pytest.raises(wm.WmbusError, match="input_agc"):
            rx.read_input_gain(0)
    # the AGC alone on plain cu8 switches the conversion kernel on
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_agc=1) as rx:
        text = rx.run(cu8)[0]
        assert rx.resampler_launches() == 1
        y, clips, g = AR.convert(cu8, FR.CU8)
        assert np.array_equal(rx.read_resampled(0), y) and np.array_equal(rx.read_input_gain(0), g)
        tm = rx.timing()
        assert tm["input_bytes_out"] == cu8.size and tm["input_clipped"] == clips == 0
        assert text == oracle.run(y, oracle.make_opts())["text"]


def test_bad_arguments_are_refused(wm):
    for bad in (2, 1 << 31):
        with pytest.raises(wm.WmbusError, match="input_agc") as e:
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_agc=bad)
        assert "(-1)" in str(e.value)                        # WMBUS_EINVAL
    for gain in (1, 255, 257, 65535):
        with pytest.raises(wm.WmbusError, match="input_agc") as e:
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_agc=1, input_gain_q8=gain)
        assert "(-1)" in str(e.value)
    with pytest.raises(wm.WmbusError, match="input_agc"):
        wm.Batch(n_streams=8, max_push_bytes=1 << 16, input_agc=1, input_gain_q8=512)
    for gain in (0, 256):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_agc=1, input_gain_q8=gain, input_format=wm.FMT_CF32):
            pass
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for bad in (["-g", "auto", "-g", "20"], ["-g", "0", "-g", "auto"], ["-g", "Auto"], ["-g", "automatic"]):
        p = subprocess.run([wm.CLI_PATH] + bad, input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-g auto" in p.stdout.decode(), bad
    p = subprocess.run([wm.CLI_PATH, "-g", "auto"], input=b"", capture_output=True, env=env)
    assert p.returncode == 0, p.stderr
