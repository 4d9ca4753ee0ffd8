"""cfg.input_dc on the GPU: the bytes, the clip count, the byte count and the dc table of k0_dc_sums -> k0_dc_plan -> the DC
instantiations of the two K0-stage kernels against the numpy restatement (tests/dc_ref.py); offset captures as cs8 at 2.048 MS/s
through a single context, a batch and the CLI print the oracle's text on the restated bytes; input_dc = 0 is the context it always
was; bad arguments."""
import os
import subprocess

import numpy as np
import pytest

import dc_ref as DR
import format_ref as FR
from lanes import one_lane
from test_dc_emulated import OUT_HZ, RATE_IDS, RATES, dc_inputs
from test_formats_emulated import FMT_IDS, FORMATS
from test_resample_emulated import BLK, CUTS, N_BLOCKS

pytestmark = pytest.mark.gpu

KINDS = 1 | 2 | 4 | 8
SHIFT = 250000


def design(wm, rate):
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, OUT_HZ)
    return L, M, taps


_WANT = {}


def restated(wm, key, raw, fmt, R, fin, f, g, rate):
    """dc_ref.convert of one capture, computed once per (input, format, R, rate, shift, gain) and shared by the cuts and windows."""
    k = key + (fmt, R, rate, f, g)
    if k not in _WANT:
        L, M, taps = design(wm, rate)
        _WANT[k] = DR.convert(raw, fmt, R, fin, f, g, L, M, taps)
    return _WANT[k]


@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven", "each-4096"])
@pytest.mark.parametrize("n_streams", [1, 8])
@pytest.mark.parametrize("R", [1, 6], ids=["R1", "R6"])
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_bytes_clip_count_and_dc_equal_the_restatement(wm, fmt, rate, R, n_streams, cut, windows):
    """A different capture per stream (the named inputs of the emulated test, then random bit patterns), so that a stride, a history
    or a state mix-up shows; gain x 1 on one stream, x 16 (random full-range input clips) on eight; the 250 kHz shift behind the
    blocker on the cs16 and cu8 cases.  each-4096 is 21 pushes: A is carried across every one of them."""
    fin = rate or OUT_HZ
    f = SHIFT if fmt in (FR.CS16, FR.CU8) else 0
    named = dc_inputs(fmt, N_BLOCKS * BLK)
    rng = np.random.default_rng(2000 * fmt + n_streams)
    names = list(named)
    caps = [named[names[s]] if s < len(names) else rng.integers(0, 256, N_BLOCKS * BLK, dtype=np.uint8) for s in range(n_streams)]
    keys = [(names[s],) if s < len(names) else ("random", n_streams, s) for s in range(n_streams)]
    g = 256 if n_streams == 1 else 4096
    with wm.Receiver(n_streams=n_streams, max_push_bytes=N_BLOCKS * BLK, input_rate_hz=rate, input_shift_hz=f, input_format=fmt, input_gain_q8=g,
                     input_dc=R, input_windows=windows) as rx:
        got, dcs, off, clipped, bytes_out = [[] for _ in caps], [[] for _ in caps], 0, 0, 0
        for n in CUTS[cut]:
            rx.push([a[off:off + n] for a in caps]); off += n
            for s in range(n_streams):
                got[s].append(rx.read_resampled(s))
                dc = rx.read_input_dc(s)
                assert dc.shape == (n // FR.BPS[fmt] // DR.BLOCK, 2)
                dcs[s].append(dc.astype(np.int64))
            tm = rx.timing()
            clipped += tm["input_clipped"]; bytes_out += tm["input_bytes_out"]
        assert rx.resampler_launches() == len(CUTS[cut])
    want_clips = 0
    for s in range(n_streams):
        y, clips, dc = restated(wm, keys[s], caps[s], fmt, R, fin, f, g, rate)
        want = y[:y.size // BLK * BLK]
        have, have_dc = np.concatenate(got[s]), np.concatenate(dcs[s])
        assert np.array_equal(have_dc, dc), (s, int(np.argmax(np.any(have_dc != dc, axis=1))))
        assert have.size == want.size, s
        assert np.array_equal(have, want), (s, int(np.argmax(have != want)))
        want_clips += clips
    assert clipped == want_clips
    assert bytes_out == n_streams * restated(wm, keys[0], caps[0], fmt, R, fin, f, g, rate)[0].size


_OFFSET = {}
OFFSET_KW = dict(input_rate_hz=2048000, input_format=FR.CS8, input_dc=6)


def offset_captures(wm, oracle):
    """The three offset cs8 captures and the oracle's text on tests/dc_ref.py's bytes of each: computed once, shared, left unchanged."""
    if not _OFFSET:
        L, M, T, taps = wm.resampler_design(2048000, OUT_HZ)
        cu8s = [wm.synth_capture(seed=8300 + s, n_samples=1 << 20, fs_khz=2048, kinds=KINDS, frames_per_s=60.0, amplitude=20.0, noise_sigma=3.0)[0] for s in range(3)]
        caps = [FR.raw_bytes(DR.add_offset_cu8(c, 12, -9).astype(np.int64) - 128, FR.CS8) for c in cu8s]
        want = [oracle.run(DR.pipeline_bytes(c, FR.CS8, 6, 2048000, 0, 256, L, M, taps), oracle.make_opts())["text"] for c in caps]
        assert all(len(w.splitlines()) >= 10 for w in want)
        for c in caps:
            c.setflags(write=False)
        _OFFSET.update(caps=caps, want=want)
    return _OFFSET["caps"], _OFFSET["want"]


def test_offset_cs8_captures_in_one_lane(wm, oracle):
    """The batch of the test below as two contexts of two captures in ONE lane (the fourth capture is the first again), four pushes of
    2^19 bytes: k0_dc_sums, k0_dc_plan and the DC form of the input kernel recorded and issued behind the mate's operations."""
    caps, want = offset_captures(wm, oracle)
    got = one_lane(wm, caps + [caps[0]], 4, push=1 << 19, n_push=caps[0].size >> 19, input_windows=2, **OFFSET_KW)
    assert got.plan == [(0, 2), (2, 2)] and caps[0].size >> 19 == 4
    assert [got.whole_text(s) for s in range(4)] == want + [want[0]]


def test_offset_cs8_captures_give_the_oracles_text_on_the_restated_bytes(wm, oracle):
    """Three 2.048 MS/s synthetic captures of medium strength (amplitude 20 cu8 steps) with an I/Q offset of (+12, -9) added, written as
    cs8: a single context in one push and in odd pushes, a batch and the CLI (-I cs8 -R 2.048M -C 6 -v) print what the oracle prints
    on tests/dc_ref.py's bytes."""
    L, M, T, taps = wm.resampler_design(2048000, OUT_HZ)
    caps, want = offset_captures(wm, oracle)
    opts = oracle.make_opts()
    # the blocker is what receives them
    assert oracle.run(FR.pipeline_bytes(caps[0], FR.CS8, 256, L, M, taps), opts)["text"] != want[0]
    kw = OFFSET_KW
    with wm.Receiver(n_streams=3, max_push_bytes=caps[0].size, **kw) as rx:
        assert rx.run(caps) == want
        dc = rx.read_input_dc(0)
        assert dc.shape == ((1 << 20) // DR.BLOCK, 2) and np.abs(dc[64:] - np.array([24, -18])).max() <= 2      # 2 x the byte offset in units of x; half a unit of rounding, the bursts average out below one
    with wm.Receiver(n_streams=3, max_push_bytes=1 << 19, input_windows=2, keep_taps=False, **kw) as rx:
        assert rx.run(caps, push_bytes=BLK * 97) == want
        assert rx.read_input_dc(2).shape[0] > 0              # the offset's feedback needs no debug views
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
        assert st["samples"] == 3 * caps[0].size // 2
    assert text == want
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    p = subprocess.run([wm.CLI_PATH, "-I", "cs8", "-R", "2.048M", "-C", "6", "-v", "-B", str(1 << 19)], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == want[0]


def test_dc_zero_is_the_plain_path_and_dc_alone_is_a_stage(wm, oracle):
    cu8 = wm.synth_capture(seed=12, n_samples=1 << 18, kinds=KINDS, frames_per_s=60.0)[0]
    want = oracle.run(cu8, oracle.make_opts())["text"]
    assert len(want.splitlines()) >= 5
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_dc=0) as rx:
        assert rx.run(cu8)[0] == want
        assert rx.resampler_launches() == 0
        tm = rx.timing()
        assert tm["input_clipped"] == 0 and tm["input_bytes_out"] == 0
        with pytest.raises(wm.WmbusError, match="input_dc"):
            rx.read_input_dc(0)
        with pytest.raises(wm.WmbusError):
            rx.read_resampled(0)
    # a context that converts without the blocker has no dc to read either
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_format=wm.FMT_CS8) as rx:
        rx.push([FR.embed(cu8, FR.CS8)])
        with pytest.raises(wm.WmbusError, match="input_dc"):
            rx.read_input_dc(0)
    # the blocker alone on plain cu8 switches the conversion kernel on
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_dc=6) as rx:
        text = rx.run(cu8)[0]
        assert rx.resampler_launches() == 1
        y, clips, dc = DR.convert(cu8, FR.CU8, 6)
        assert np.array_equal(rx.read_resampled(0), y) and np.array_equal(rx.read_input_dc(0), dc)
        tm = rx.timing()
        assert tm["input_bytes_out"] == cu8.size and tm["input_clipped"] == clips
        assert text == oracle.run(y, oracle.make_opts())["text"]


def test_bad_arguments_are_refused(wm):
    for bad in (13, 1 << 31):
        with pytest.raises(wm.WmbusError, match="input_dc") as e:
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_dc=bad)
        assert "(-1)" in str(e.value)                        # WMBUS_EINVAL
    with pytest.raises(wm.WmbusError, match="input_dc"):
        wm.Batch(n_streams=8, max_push_bytes=1 << 16, input_dc=13)
    for ok in (1, 12):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, input_dc=ok, input_format=wm.FMT_CF32):
            pass
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    for bad in (["-C", "x"], ["-C", "0"], ["-C", "13"], ["-C", "6.5"], ["-C", ""]):
        p = subprocess.run([wm.CLI_PATH] + bad, input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode() and "-C R" in p.stdout.decode(), bad
    p = subprocess.run([wm.CLI_PATH, "-C", "6"], input=b"", capture_output=True, env=env)
    assert p.returncode == 0, p.stderr
