"""cfg.input_shift_hz on the GPU: the bytes and the clip count of the rotating instantiations of the two K0-stage kernels against the
numpy restatement (tests/shift_ref.py); a capture mixed up by 200 kHz in double and brought back by the shift prints the committed
golden (single context and CLI); resampling x shift x text against the oracle on the restated bytes; shift 0 is the context it always
was; bad arguments."""
import json
import os
import subprocess

import numpy as np
import pytest

import format_ref as FR
import shift_ref as SR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS
from test_resample_emulated import BLK, CUTS, N_BLOCKS
from test_shift_emulated import shift_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
KINDS = 1 | 2 | 4 | 8
OUT_HZ = 1600000
RATES = [0, 2048000, 2500000]
SHIFTS = [200000, -123457]


def design(wm, rate):
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, OUT_HZ)
    return L, M, taps


@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven"])
@pytest.mark.parametrize("n_streams", [1, 8])
@pytest.mark.parametrize("f", SHIFTS, ids=["+200000", "-123457"])
@pytest.mark.parametrize("rate", RATES, ids=[str(r) if r else "native" for r in RATES])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_shifted_bytes_and_clip_count_equal_the_restatement(wm, fmt, rate, f, n_streams, cut, windows):
    """A different capture per stream (the named inputs of the emulated test, then random bit patterns), so that a stride or a
    history mix-up shows; gain x 1 on one stream, x 16 (random full-range input clips) on eight."""
    L, M, taps = design(wm, rate)
    fin = rate or OUT_HZ
    named = shift_inputs(fmt, N_BLOCKS * BLK)
    rng = np.random.default_rng(1000 * fmt + n_streams)
    names = list(named)
    caps = [named[names[s]] if s < len(names) else rng.integers(0, 256, N_BLOCKS * BLK, dtype=np.uint8) for s in range(n_streams)]
    g = 256 if n_streams == 1 else 4096
    with wm.Receiver(n_streams=n_streams, max_push_bytes=N_BLOCKS * BLK, input_rate_hz=rate, input_shift_hz=f, input_format=fmt, input_gain_q8=g,
                     input_windows=windows) as rx:
        got, off, clipped, bytes_out = [[] for _ in caps], 0, 0, 0
        for n in CUTS[cut]:
            rx.push([a[off:off + n] for a in caps]); off += n
            for s in range(n_streams):
                got[s].append(rx.read_resampled(s))
            tm = rx.timing()
            clipped += tm["input_clipped"]; bytes_out += tm["input_bytes_out"]
        assert rx.resampler_launches() == len(CUTS[cut])
    want_clips = 0
    for s in range(n_streams):
        y, clips = SR.convert(caps[s], fmt, fin, f, g, L, M, taps)
        want = y[:y.size // BLK * BLK]
        have = np.concatenate(got[s])
        assert have.size == want.size, s
        assert np.array_equal(have, want), (s, int(np.argmax(have != want)))
        want_clips += clips
    assert clipped == want_clips
    assert bytes_out == n_streams * SR.convert(caps[0], fmt, fin, f, g, L, M, taps)[0].size


def test_cs16_round_trip_prints_the_golden(wm, oracle, samples):
    """samples2 mixed up by 200 kHz in double, written as cs16: with input_shift_hz = 200000 and gain 364 / 256 every byte of the
    original comes back (tests/test_shift_emulated.py), so wmbus_open ... wmbus_collect print the committed golden.  The CLI spells
    the gain in dB, which need not be Q8 364 exactly: its text is compared with the oracle's on the restated bytes of ITS gain."""
    f, cu8 = 200000, samples["samples2"]
    raw = SR.round_trip_cs16(cu8, OUT_HZ, f)
    want = BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    assert len(want.splitlines()) >= 4
    push = 1 << 20
    with wm.Receiver(n_streams=1, max_push_bytes=push, input_format=FR.CS16, input_gain_q8=SR.CS16_ROUND_TRIP_GAIN, input_shift_hz=f) as rx:
        assert rx.run(raw)[0] == want
        assert rx.resampler_launches() == raw.size // push
        assert np.array_equal(rx.read_resampled(0), cu8[-push // 2:])        # the last push's bytes: the capture's
        assert rx.timing()["input_clipped"] == 0
    db = "3.06"
    g_cli = int(np.rint(256.0 * 10.0 ** (float(db) / 20.0)))                 # wm_main.c, -g
    assert abs(g_cli - SR.CS16_ROUND_TRIP_GAIN) <= 1
    want_cli = oracle.run(SR.pipeline_bytes(raw, FR.CS16, OUT_HZ, f, g_cli), oracle.make_opts())["text"]
    assert len(want_cli.splitlines()) >= 4
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for spelled in ("200k", "0.2M", "200000"):
        p = subprocess.run([wm.CLI_PATH, "-O", spelled, "-I", "cs16", "-g", db, "-v"], input=raw.tobytes(), capture_output=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr
        assert p.stdout.decode() == want_cli, spelled


def test_resampled_and_shifted_cs16_capture_gives_the_oracles_text_on_the_restated_bytes(wm, oracle, tmp_path):
    """2.5 MS/s synthetic captures, mixed up by 250 kHz (and one down by 123 457 Hz through the CLI), written as cs16 6 bits down and
    brought back by the shift and a gain of 64: single context in one push and in odd pushes, batch files through the CLI."""
    fin, f = 2500000, 250000
    L, M, T, taps = wm.resampler_design(fin, OUT_HZ)
    g, db = 64 * 256, "36.1236"                          # 20 log10(64) = 36.1236: rint(256 * 10^(dB / 20)) = 16384
    cu8s = [wm.synth_capture(seed=8200 + s, n_samples=1 << 19, fs_khz=2500, kinds=KINDS, frames_per_s=60.0)[0] for s in range(2)]

    def mixed(c, shift):
        z = 2.0 * SR.mixed_up(c, fin, shift)             # 128 / 64 counts per cu8 half-step
        return FR.raw_bytes(np.rint(np.stack([z.real, z.imag], axis=1)).reshape(-1).astype(np.int16), FR.CS16)
    caps = [mixed(c, f) for c in cu8s]
    opts = oracle.make_opts()
    want = [oracle.run(SR.pipeline_bytes(c, FR.CS16, fin, f, g, L, M, taps), opts)["text"] for c in caps]
    assert all(len(w.splitlines()) >= 5 for w in want)
    # the shift is what receives them: unshifted, the same bytes decode to something else
    assert oracle.run(FR.pipeline_bytes(caps[0], FR.CS16, g, L, M, taps), opts)["text"] != want[0]
    kw = dict(input_rate_hz=fin, input_format=FR.CS16, input_gain_q8=g, input_shift_hz=f)
    with wm.Receiver(n_streams=2, max_push_bytes=caps[0].size, **kw) as rx:
        assert rx.run(caps) == want
    with wm.Receiver(n_streams=2, max_push_bytes=1 << 18, input_windows=2, keep_taps=False, **kw) as rx:
        assert rx.run(caps, push_bytes=BLK * 37) == want
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    p = subprocess.run([wm.CLI_PATH, "-R", "2.5M", "-O", "250k", "-I", "cs16", "-g", db, "-v", "-B", str(1 << 18)], input=caps[0].tobytes(),
                       capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == want[0]
    # batch mode with a negative offset; the shorter file is padded with the format's raw silence (0)
    f2 = -123457
    low = [mixed(c, f2) for c in cu8s]
    low[0].tofile(tmp_path / "a.cs16"); low[1][:1 << 20].tofile(tmp_path / "b.cs16")
    pad = np.concatenate([low[1][:1 << 20], np.zeros(low[0].size - (1 << 20), np.uint8)])
    want_b = {"a.cs16": oracle.run(SR.pipeline_bytes(low[0], FR.CS16, fin, f2, g, L, M, taps), opts)["text"],
              "b.cs16": oracle.run(SR.pipeline_bytes(pad, FR.CS16, fin, f2, g, L, M, taps), opts)["text"]}
    assert len(want_b["a.cs16"].splitlines()) >= 5
    p = subprocess.run([wm.CLI_PATH, "-R", "2.5M", "-O", "-123457", "-I", "cs16", "-g", db, "-v", "-G", "0", "-B", str(1 << 18), "a.cs16", "b.cs16"],
                       cwd=tmp_path, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    got = {"a.cs16": "", "b.cs16": ""}
    for line in p.stdout.decode().splitlines(True):
        name, rest = line.split(": ", 1)
        got[name] += rest
    assert got == want_b


def test_shifted_captures_in_one_batch_lane(wm, oracle):
    """The stage in a batch lane: two 2.5 MS/s captures mixed up by 250 kHz as cs16, each in both of two contexts that share ONE lane,
    eight pushes of 2^18 bytes -- the rotating input kernel recorded and issued behind the mate's operations.  Lines against the oracle on
    tests/shift_ref.py's bytes and against the lane-per-context run."""
    fin, f, g = 2500000, 250000, 64 * 256
    L, M, T, taps = wm.resampler_design(fin, OUT_HZ)
    caps = []
    for s in range(2):
        z = 2.0 * SR.mixed_up(wm.synth_capture(seed=8200 + s, n_samples=1 << 19, fs_khz=2500, kinds=KINDS, frames_per_s=60.0)[0], fin, f)
        caps.append(FR.raw_bytes(np.rint(np.stack([z.real, z.imag], axis=1)).reshape(-1).astype(np.int16), FR.CS16))
    want = [oracle.run(SR.pipeline_bytes(c, FR.CS16, fin, f, g, L, M, taps), oracle.make_opts())["text"] for c in caps]
    assert all(len(w.splitlines()) >= 5 for w in want)
    got = one_lane(wm, caps + caps, 4, push=1 << 18, n_push=caps[0].size >> 18, input_windows=2, input_rate_hz=fin, input_format=FR.CS16, input_gain_q8=g,
                   input_shift_hz=f)
    assert got.plan == [(0, 2), (2, 2)] and caps[0].size >> 18 == 8
    assert [got.whole_text(s) for s in range(4)] == want + want


def test_shift_zero_is_the_plain_path_and_a_shift_alone_is_a_stage(wm, oracle):
    cu8 = wm.synth_capture(seed=12, n_samples=1 << 18, kinds=KINDS, frames_per_s=60.0)[0]
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size) as rx:
        want = rx.run(cu8)[0]
    assert want == oracle.run(cu8, oracle.make_opts())["text"] and len(want.splitlines()) >= 5
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_shift_hz=0) as rx:
        assert rx.run(cu8)[0] == want
        assert rx.resampler_launches() == 0
        tm = rx.timing()
        assert tm["input_clipped"] == 0 and tm["input_bytes_out"] == 0
        with pytest.raises(wm.WmbusError):
            rx.read_resampled(0)
    # a shift alone on plain cu8 switches the conversion kernel on: debug read, byte count and clip count work
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_shift_hz=1) as rx:
        text = rx.run(cu8)[0]
        assert rx.resampler_launches() == 1
        y, clips = SR.convert(cu8, FR.CU8, OUT_HZ, 1)
        assert np.array_equal(rx.read_resampled(0), y)
        tm = rx.timing()
        assert tm["input_bytes_out"] == cu8.size and tm["input_clipped"] == clips
        assert text == oracle.run(y, oracle.make_opts())["text"]


def test_bad_arguments_are_refused(wm):
    for kw, limit in ((dict(input_shift_hz=800001), "800000"), (dict(input_shift_hz=-800001), "800000"),
                      (dict(input_shift_hz=1024001, input_rate_hz=2048000), "1024000"),
                      (dict(input_shift_hz=-1200001, decimation=3), "1200000")):
        with pytest.raises(wm.WmbusError, match="input_shift_hz") as e:
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw)
        assert "(-1)" in str(e.value) and limit in str(e.value), str(e.value)      # WMBUS_EINVAL, and the message names the limit
    with pytest.raises(wm.WmbusError, match="input_shift_hz"):
        wm.Batch(n_streams=8, max_push_bytes=1 << 16, input_shift_hz=800001)
    for kw in (dict(input_shift_hz=800000), dict(input_shift_hz=-800000), dict(input_shift_hz=-1024000, input_rate_hz=2048000, input_format=wm.FMT_CF32)):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw):
            pass
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for bad in (["-O", "foo"], ["-O", "250kHz"], ["-O", "--5"], ["-O", ""]):
        p = subprocess.run([wm.CLI_PATH] + bad, input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-O Hz" in p.stdout.decode(), bad
    p = subprocess.run([wm.CLI_PATH, "-O", "900k"], input=b"", capture_output=True, env=env)
    assert p.returncode == 1 and b"800000" in p.stderr
    p = subprocess.run([wm.CLI_PATH, "-O", "0"], input=b"", capture_output=True, env=env)
    assert p.returncode == 0, p.stderr
