"""cfg.input_format / cfg.input_gain_q8 on the GPU: the bytes of the two K0-stage kernels (the resampler's format paths, the
conversion-only kernel) and the clip counter against the numpy restatement (tests/format_ref.py); every bundled golden through the
new paths (a cu8 capture embedded in a wider format decodes to the same text: single context, wmbus_batch, CLI); resampling x
format x text against the oracle on the restated bytes; the untouched cu8 path; bad arguments."""
import json
import os
import subprocess

import numpy as np
import pytest

import format_ref as FR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS, design_inputs, inputs
import resample_ref as RR
from test_resample_emulated import BLK, CUTS, N_BLOCKS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
KINDS = 1 | 2 | 4 | 8
RATES = [0, 2048000, 2500000]
WIDE = [FR.CS8, FR.CS16, FR.CF32]
WIDE_IDS = [FR.NAMES[f] for f in WIDE]
# (sample key, golden key, Receiver keywords, CLI switches)
GOLDENS = [("samples2", "rtlsdr_868.950M_1M6_samples2.cu8|-v", dict(), ["-v"]),
           ("issue48", "rtlsdr_868.625M_2M4_issue48.cu8|-d 3 -s -v", dict(decimation=3, simultaneous=True), ["-d", "3", "-s", "-v"])]
GOLDEN_IDS = ["samples2", "issue48"]


def design(wm, rate):
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, 1600000)
    return L, M, taps


@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven"])
@pytest.mark.parametrize("n_streams", [1, 8])
@pytest.mark.parametrize("rate", RATES, ids=[str(r) if r else "native" for r in RATES])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_converted_bytes_and_clip_count_equal_the_restatement(wm, fmt, rate, n_streams, cut, windows):
    L, M, taps = design(wm, rate)
    named = inputs(fmt, N_BLOCKS * BLK)
    rng = np.random.default_rng(1000 * fmt + n_streams)
    names = list(named)                                      # random first; then minimum, maximum, (cf32: wide, special values), ...
    caps = [named[names[s]] if s < len(names) else rng.integers(0, 256, N_BLOCKS * BLK, dtype=np.uint8)      # ... and random BIT patterns
            for s in range(n_streams)]
    for g in (256, 4096):
        if fmt == FR.CU8 and rate == 0 and g == 256:
            continue                                         # the plain cu8 path: no stage at all (tested below)
        with wm.Receiver(n_streams=n_streams, max_push_bytes=N_BLOCKS * BLK, input_rate_hz=rate, input_format=fmt, input_gain_q8=g,
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
            y, clips = FR.convert(caps[s], fmt, g, L, M, taps)
            want = y[:y.size // BLK * BLK]
            have = np.concatenate(got[s])
            assert have.size == want.size, (g, s)
            assert np.array_equal(have, want), (g, s, int(np.argmax(have != want)))
            want_clips += clips
        assert clipped == want_clips, g
        assert bytes_out == n_streams * FR.convert(caps[0], fmt, g, L, M, taps)[0].size, g


def corner_cases():
    """cu8 and cf32 at every corner; all four formats at the T = 512 corners and at 16 / 1."""
    out = []
    for fin, d in RR.CORNERS:
        L, M, T = RR.geometry(fin, d)
        for fmt in (FORMATS if T == 512 or (L, M) == (16, 1) else [FR.CU8, FR.CF32]):
            out.append(pytest.param(fin, d, fmt, id=f"{fin}-d{d}-{FR.NAMES[fmt]}"))
    return out


@pytest.mark.parametrize("fin,d,fmt", corner_cases())
def test_corners_bytes_and_clip_count_equal_the_restatement(wm, fin, d, fmt):
    """The compiled kernels at the corners of the design space (tests/resample_ref.py::CORNERS): 1 stream at gain x 1 and 8 streams
    (random, minimum, maximum, square wave, random bit patterns) at x 16, one and two input windows, one push and 4096-byte pushes
    (cf32 at T = 512: 512 samples against a history of 511).  max_push_bytes is the length of the one push, so at 16 / 1 and
    decimation 16 the pipeline behind the resampler is sized by what a full raw push resamples to (push_cap in wmbus_open), 16 times
    the raw push."""
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    n_bytes = RR.blocks_input(L, M, FR.BPS[fmt])
    cuts = RR.cuts_for(n_bytes)
    named = design_inputs(fmt, n_bytes, T)
    rng = np.random.default_rng(fin + fmt)
    for n_streams, g in ((1, 256), (8, 4096)):
        caps = [named[k] for k in list(named)[:n_streams]] + [rng.integers(0, 256, n_bytes, dtype=np.uint8) for _ in range(n_streams - 4)]
        want = [FR.convert(c, fmt, g, L, M, taps) for c in caps]
        assert all(w[0].size // BLK >= 3 for w in want)
        for windows in (1, 2):
            for cut in ("one", "each-4096"):
                with wm.Receiver(n_streams=n_streams, max_push_bytes=n_bytes, decimation=d, input_rate_hz=fin, input_format=fmt, input_gain_q8=g,
                                 input_windows=windows) as rx:
                    got, off, clipped, bytes_out = [[] for _ in caps], 0, 0, 0
                    for n in cuts[cut]:
                        rx.push([a[off:off + n] for a in caps]); off += n
                        for s in range(n_streams):
                            got[s].append(rx.read_resampled(s, cap=BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M)))
                        tm = rx.timing()
                        clipped += tm["input_clipped"]; bytes_out += tm["input_bytes_out"]
                    assert rx.resampler_launches() == len(cuts[cut])
                for s in range(n_streams):
                    y = want[s][0]
                    have = np.concatenate(got[s])
                    assert have.size == y.size // BLK * BLK, (n_streams, windows, cut, s)
                    assert np.array_equal(have, y[:have.size]), (n_streams, windows, cut, s, int(np.argmax(have != y[:have.size])))
                assert clipped == sum(w[1] for w in want), (n_streams, windows, cut)
                assert bytes_out == sum(w[0].size for w in want), (n_streams, windows, cut)


@pytest.mark.parametrize("sample,key,kw,cli", GOLDENS, ids=GOLDEN_IDS)
@pytest.mark.parametrize("fmt", WIDE, ids=WIDE_IDS)
def test_bundled_goldens_through_the_new_formats(wm, samples, fmt, sample, key, kw, cli, tmp_path):
    """The reference's own stdout on the bundled recordings, byte for byte, from the recording embedded in another format."""
    cu8 = samples[sample]
    cu8 = cu8[:cu8.size // BLK * BLK]
    raw = FR.embed(cu8, fmt)
    want = BUNDLED[key]
    assert len(want.splitlines()) >= 1
    push = 1 << 20
    # single context
    with wm.Receiver(n_streams=1, max_push_bytes=push, input_format=fmt, **kw) as rx:
        assert rx.run(raw)[0] == want
        assert rx.resampler_launches() == (raw.size + push - 1) // push
    # the CLI on stdin
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    p = subprocess.run([wm.CLI_PATH, "-I", FR.NAMES[fmt]] + cli, input=raw.tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == want
    # wmbus_batch, 8 streams, host-sourced
    text = [""] * 8
    with wm.Batch(n_streams=8, max_push_bytes=push, input_format=fmt, input_windows=2, **kw) as b:
        pos = {}

        def fill(first, n, slab):
            off = pos.get(first, 0)
            k = min(push, raw.size - off)
            for s in range(n):
                slab[s, :k] = raw[off:off + k]
            pos[first] = off + k
            return k

        def on_push(first, n, lines, tm):
            assert tm["input_clipped"] == 0
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        st = b.run_from(fill, on_push)
        assert st["samples"] == 8 * cu8.size // 2            # samples, whatever their raw size
    assert text == [want] * 8


@pytest.mark.parametrize("sample,key,kw,cli", GOLDENS, ids=GOLDEN_IDS)
@pytest.mark.parametrize("fmt", WIDE, ids=WIDE_IDS)
def test_bundled_goldens_in_one_lane(wm, samples, fmt, sample, key, kw, cli):
    """The batch of the test above as two contexts of four streams in ONE lane: the format's input kernel recorded and issued behind the
    mate's operations, in pushes of 2^20 raw bytes, or of half the recording where that is less (two pushes at least: a carry)."""
    cu8 = samples[sample]
    cu8 = cu8[:cu8.size // BLK * BLK]
    raw = FR.embed(cu8, fmt)
    want = BUNDLED[key]
    assert len(want.splitlines()) >= 1
    push = min(1 << 20, raw.size // 2 // BLK * BLK)
    sizes = [min(push, raw.size - off) for off in range(0, raw.size, push)]
    assert len(sizes) >= 2
    got = one_lane(wm, [raw] * 8, 8, push=push, sizes_of={0: sizes, 4: sizes}, input_windows=2, input_format=fmt, **kw)
    assert got.plan == [(0, 4), (4, 4)] and all(tm["input_clipped"] == 0 for per in got.timing.values() for tm in per)
    assert [got.whole_text(s) for s in range(8)] == [want] * 8


_CS16 = {}
CS16_GAIN = 64 * 256


def cs16_captures(wm, oracle):
    """Three 2.048 MS/s captures as cs16 6 bits down and the oracle's text on the restated bytes: computed once, shared, left unchanged."""
    if not _CS16:
        L, M, T, taps = wm.resampler_design(2048000, 1600000)
        cu8s = [wm.synth_capture(seed=8100 + s, n_samples=1 << 20, fs_khz=2048, kinds=KINDS, frames_per_s=60.0)[0] for s in range(3)]
        caps = [FR.raw_bytes(FR.embed(c, FR.CS16).view("<i2") >> 6, FR.CS16) for c in cu8s]
        want = [oracle.run(FR.pipeline_bytes(c, FR.CS16, CS16_GAIN, L, M, taps), oracle.make_opts())["text"] for c in caps]
        assert all(len(w.splitlines()) >= 10 for w in want)
        for c in caps:
            c.setflags(write=False)
        _CS16.update(caps=caps, want=want)
    return _CS16["caps"], _CS16["want"]


def test_resampling_a_cs16_capture_in_one_lane(wm, oracle):
    """The batch of the test below as two contexts of two captures in ONE lane (the fourth capture is the first again), eight pushes of 2^19 bytes."""
    caps, want = cs16_captures(wm, oracle)
    got = one_lane(wm, caps + [caps[0]], 4, push=1 << 19, n_push=caps[0].size >> 19, input_windows=2, input_rate_hz=2048000, input_format=FR.CS16,
                   input_gain_q8=CS16_GAIN)
    assert got.plan == [(0, 2), (2, 2)] and caps[0].size >> 19 == 8
    assert [got.whole_text(s) for s in range(4)] == want + [want[0]]


def test_resampling_a_cs16_capture_gives_the_oracles_text_on_the_restated_bytes(wm, oracle, tmp_path):
    """2.048 MS/s synthetic captures, written as cs16 6 bits down and brought back by a gain of 64: single context, batch, CLI."""
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    g, db = CS16_GAIN, "36.1236"                         # 20 log10(64) = 36.1236: rint(256 * 10^(dB / 20)) = 16384
    caps, want = cs16_captures(wm, oracle)
    opts = oracle.make_opts()
    kw = dict(input_rate_hz=2048000, input_format=FR.CS16, input_gain_q8=g)
    with wm.Receiver(n_streams=3, max_push_bytes=caps[0].size, **kw) as rx:
        assert rx.run(caps) == want
    with wm.Receiver(n_streams=3, max_push_bytes=1 << 19, input_windows=2, keep_taps=False, **kw) as rx:
        assert rx.run(caps, push_bytes=BLK * 97) == want
    push = 1 << 19
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
    p = subprocess.run([wm.CLI_PATH, "-R", "2.048M", "-I", "cs16", "-g", db, "-v", "-B", str(1 << 19)], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == want[0]
    # batch mode: the shorter file is padded with the format's silence (0), -S reports the clipped share
    caps[0].tofile(tmp_path / "a.cs16"); caps[1][:3 << 20].tofile(tmp_path / "b.cs16")
    pad = np.concatenate([caps[1][:3 << 20], np.zeros(caps[0].size - (3 << 20), np.uint8)])
    want_b = oracle.run(FR.pipeline_bytes(pad, FR.CS16, g, L, M, taps), opts)["text"]
    p = subprocess.run([wm.CLI_PATH, "-R", "2.048M", "-I", "cs16", "-g", db, "-v", "-S", "-B", str(1 << 19), "a.cs16", "b.cs16"], cwd=tmp_path,
                       capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    got = {"a.cs16": "", "b.cs16": ""}
    for line in p.stdout.decode().splitlines(True):
        name, rest = line.split(": ", 1)
        got[name] += rest
    assert got == {"a.cs16": want[0], "b.cs16": want_b}
    assert b"bytes clipped" in p.stderr and f"{2 * caps[0].size // 4} samples".encode() in p.stderr


def test_plain_cu8_takes_no_stage_and_prints_the_same_text(wm, oracle):
    cu8 = wm.synth_capture(seed=12, n_samples=1 << 18, kinds=KINDS, frames_per_s=60.0)[0]
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size) as rx:
        want = rx.run(cu8)[0]
    assert want == oracle.run(cu8, oracle.make_opts())["text"] and len(want.splitlines()) >= 5
    for g in (0, 256):
        with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_format=wm.FMT_CU8, input_gain_q8=g, input_rate_hz=1600000) as rx:
            assert rx.run(cu8)[0] == want
            assert rx.resampler_launches() == 0
            tm = rx.timing()
            assert tm["input_clipped"] == 0 and tm["input_bytes_out"] == 0
            with pytest.raises(wm.WmbusError):
                rx.read_resampled(0)
    # a gain alone switches the conversion kernel on; x 1 spelled as a conversion gives the same text
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_format=wm.FMT_CS8) as rx:
        assert rx.run(FR.embed(cu8, FR.CS8))[0] == want
        assert rx.resampler_launches() == 1


def test_bad_arguments_are_refused(wm):
    with pytest.raises(wm.WmbusError, match="input_format"):
        wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_format=4)
    with pytest.raises(wm.WmbusError, match="input_gain_q8"):
        wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_gain_q8=65536)
    with pytest.raises(wm.WmbusError, match="input_format"):
        wm.Batch(n_streams=8, max_push_bytes=1 << 16, input_format=9)
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_gain_q8=65535, input_format=wm.FMT_CF32):
        pass
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for bad in (["-I", "foo"], ["-I", "CS16"], ["-g", "loud"], ["-g", "3dB"]):
        p = subprocess.run([wm.CLI_PATH] + bad, input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-I cu8|cs8|cs16|cf32" in p.stdout.decode(), bad
