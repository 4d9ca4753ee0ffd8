"""Sample formats and input gain (cfg.input_format, cfg.input_gain_q8): the device source of the two K0-stage kernels
(rtl-wmbus_amd/csrc/wm_k0_resample.h: the resampler's format loaders and output stage, the conversion-only kernel) on the coroutine
block emulator against the numpy restatement tests/format_ref.py, byte for byte and clip count for clip count; the embedding identity
that makes every cu8 golden a test of the new paths; and what the gain is for, through the oracle.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import format_ref as FR
import resample_ref as RR
from test_resample_emulated import BLK, CUTS, N_BLOCKS, N_YIELD, received, yield_captures

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libformat_emu.so")
SRC = os.path.join(HERE, "emu", "format_emu.cpp")

FORMATS = [FR.CU8, FR.CS8, FR.CS16, FR.CF32]
FMT_IDS = [FR.NAMES[f] for f in FORMATS]
RATES = [0, 2048000, 2500000, 10000000]                # 0: already at 1.6 MS/s, the conversion kernel; else the resampler to 1.6 MS/s
GAINS = [256, 1, 4096, 65535]
WIDE = [FR.CS8, FR.CS16, FR.CF32]


def test_the_abi_has_the_format_fields(wm):
    """Fails on a tree without the feature: no input_format / input_gain_q8 in the configuration, no clip counter in the timing."""
    names = [f[0] for f in wm.Cfg._fields_]
    assert names[-2:] == ["input_format", "input_gain_q8"]              # at the END: zero-initialised and older callers are unchanged
    assert [f[0] for f in wm.Timing._fields_][-2:] == ["input_bytes_out", "input_clipped"]
    assert (wm.FMT_CU8, wm.FMT_CS8, wm.FMT_CS16, wm.FMT_CF32) == (FR.CU8, FR.CS8, FR.CS16, FR.CF32)
    c = wm.Cfg()
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_format == 0 and c.input_gain_q8 == 0
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h")).read()
    for word in ("WMBUS_FMT_CU8 = 0", "WMBUS_FMT_CS8", "WMBUS_FMT_CS16", "WMBUS_FMT_CF32", "input_gain_q8", "input_clipped"):
        assert word in hdr, word


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_fmt_new.restype = ctypes.c_void_p
    L.wm_emu_fmt_new.argtypes = [ctypes.c_uint] * 5 + [ctypes.c_void_p, ctypes.c_uint]
    L.wm_emu_fmt_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_fmt_push.restype = ctypes.c_long
    L.wm_emu_fmt_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_fmt_bps.restype = ctypes.c_uint
    L.wm_emu_fmt_bps.argtypes = [ctypes.c_uint]
    L.wm_emu_fmt_pick_tile.restype = ctypes.c_uint
    L.wm_emu_fmt_pick_tile.argtypes = [ctypes.c_uint] * 3
    L.wm_emu_fmt_start_at.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    L.wm_emu_fmt_convert_tile.restype = ctypes.c_uint
    L.wm_emu_fmt_convert_tile.argtypes = [ctypes.c_uint]
    return L


def design(wm, rate):
    """(L, M, taps) of the path `rate` takes at decimation 2; taps None: the conversion kernel."""
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, 1600000)
    return L, M, taps


def run_emulated(emu, raw, fmt, gain, L, M, taps, cuts, tile, start_at=None):
    """(the bytes the pipeline takes, push by push, concatenated; the clip counts of the pushes summed).  start_at: (input samples,
    outputs) the stream already has behind it, all of them x = 0."""
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_fmt_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile)
    if start_at is not None:
        emu.wm_emu_fmt_start_at(h, start_at[0], start_at[1])
    got, off, clipped = [], 0, 0
    try:
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            win = np.full(BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M) + 64, 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            r = emu.wm_emu_fmt_push(h, part.ctypes.data, part.size, win.ctypes.data, win.size - 64, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[-64:] == 0xA5)                 # nothing written past the window
            got.append(win[:r].copy()); clipped += clip.value
    finally:
        emu.wm_emu_fmt_free(h)
    assert off == raw.size
    return np.concatenate(got), clipped


def library_tile(emu, wm, fmt, rate):
    """The tile wmbus_open picks for the path."""
    if rate == 0:
        return emu.wm_emu_fmt_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, 1600000)
    tile = emu.wm_emu_fmt_pick_tile(L, M, T)
    assert tile > 0
    return tile


CF32_ROW = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0,
                     32767.5 / 32768, -32768.5 / 32768, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1.00001, -1.00001,
                     7.0, -7.0, 3.4e38, -3.4e38, 0.25, -0.25, 100.5 / 32768, 101.5 / 32768, 1e-5, -1e-5, 0.999], np.float32)


def inputs(fmt, n_bytes):
    """Raw byte streams of n_bytes: random over the format's full range, all-minimum, all-maximum; cf32 also a row of special values."""
    rng = np.random.default_rng(0xF0 + fmt)
    n = n_bytes // (FR.BPS[fmt] // 2)                    # values (I and Q count separately)
    if fmt == FR.CU8:
        return {"random": FR.raw_bytes(rng.integers(0, 256, n), fmt), "min": FR.raw_bytes(np.zeros(n), fmt), "max": FR.raw_bytes(np.full(n, 255), fmt)}
    if fmt == FR.CS8:
        return {"random": FR.raw_bytes(rng.integers(-128, 128, n), fmt), "min": FR.raw_bytes(np.full(n, -128), fmt), "max": FR.raw_bytes(np.full(n, 127), fmt)}
    if fmt == FR.CS16:
        return {"random": FR.raw_bytes(rng.integers(-32768, 32768, n), fmt), "min": FR.raw_bytes(np.full(n, -32768), fmt),
                "max": FR.raw_bytes(np.full(n, 32767), fmt)}
    special = np.resize(CF32_ROW, n)
    return {"random": FR.raw_bytes(rng.uniform(-1.0, 1.0, n), fmt), "min": FR.raw_bytes(np.full(n, -1.0), fmt), "max": FR.raw_bytes(np.full(n, 1.0), fmt),
            "wide": FR.raw_bytes(rng.normal(0.0, 0.7, n), fmt), "special": FR.raw_bytes(special, fmt)}


def test_cf32_rounding_rule():
    """The one float step of the contract, value by value."""
    x = FR.to_x(FR.raw_bytes(CF32_ROW, FR.CF32), FR.CF32).reshape(-1)
    want = [0, 0, 32767, -32768, 0, 0, 0, 0, 0, 0, 32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 32767, -32768,
            8192, -8192, 100, 102, 0, 0, 32735]
    assert x.tolist() == want


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("rate", RATES, ids=[str(r) if r else "native" for r in RATES])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fmt, rate, cut):
    L, M, taps = design(wm, rate)
    tile = library_tile(emu, wm, fmt, rate)
    clip_seen = 0
    for name, raw in inputs(fmt, N_BLOCKS * BLK).items():
        for g in GAINS:
            want, clips = FR.convert(raw, fmt, g, L, M, taps)
            want = want[:want.size // BLK * BLK]
            got, got_clips = run_emulated(emu, raw, fmt, g, L, M, taps, CUTS[cut], tile)
            assert got.size == want.size, (name, g)
            assert np.array_equal(got, want), (name, g, int(np.argmax(got != want)))
            assert got_clips == clips, (name, g)             # every output counted, the ones behind the last whole block too
            clip_seen += clips
    assert clip_seen > 0                                     # the clamp is reached


@pytest.mark.parametrize("rate", RATES, ids=[str(r) if r else "native" for r in RATES])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_result_does_not_depend_on_the_tile(emu, wm, fmt, rate):
    """Small tiles: many blocks per push, block edges at every phase."""
    L, M, taps = design(wm, rate)
    raw = inputs(fmt, N_BLOCKS * BLK)["random"]
    for g in (256, 4096):
        want, clips = FR.convert(raw, fmt, g, L, M, taps)
        want = want[:want.size // BLK * BLK]
        for tile in ((8, 72, 1000) if rate == 0 else (64, 190)):
            got, got_clips = run_emulated(emu, raw, fmt, g, L, M, taps, CUTS["uneven"], tile)
            assert np.array_equal(got, want) and got_clips == clips, (g, tile)


SMALL_TILE = 190                                    # not a multiple of any 4 L: every block ends in a partial group
CLIP_GAIN = 4096                                    # x 16: random full-range input clips


def design_inputs(fmt, n_bytes, T):
    """random, all-minimum, all-maximum of inputs() and the full-scale square wave of 3 T samples per half period, in the format."""
    named = inputs(fmt, n_bytes)
    lo, hi = {FR.CU8: (0, 255), FR.CS8: (-128, 127), FR.CS16: (-32768, 32767), FR.CF32: (-1.0, 1.0)}[fmt]
    n = n_bytes // FR.BPS[fmt]
    sq = np.repeat(np.where((np.arange(n) // (3 * T)) % 2 == 0, lo, hi), 2)
    return {"random": named["random"], "min": named["min"], "max": named["max"], "square": FR.raw_bytes(sq, fmt)}


FULL = os.environ.get("WMBUS_RESAMPLE_FULL") == "1"


def check_design_on_the_emulator(emu, wm, fin, d, fmt, full=True):
    """One design and format, bytes and clip counts.  Inputs random, all-minimum, all-maximum and the square wave at gain x 1, the
    random one at x 16 as well; each under one push, the uneven cut and 4096-byte pushes with the library's tile; the random one
    also with the small odd tile under the uneven cut.  full=False (the drawn designs, unless WMBUS_RESAMPLE_FULL=1): random and
    square only, 4096-byte pushes with the library's tile and the uneven cut with the small one.  The input is sized so that the
    pipeline gets at least three whole blocks.  A 4096-byte cf32 push is 512 samples: at T = 512 one more than the history the next
    push needs."""
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    assert (L, M, T) == RR.geometry(fin, d)
    tile = emu.wm_emu_fmt_pick_tile(L, M, T)
    assert tile > 0
    n_bytes = RR.blocks_input(L, M, FR.BPS[fmt])
    cuts = RR.cuts_for(n_bytes)
    assert min(cuts["each-4096"]) // FR.BPS[fmt] > T - 1
    clip_seen = 0
    for name, raw in design_inputs(fmt, n_bytes, T).items():
        if not full and name not in ("random", "square"):
            continue
        for g in (256, CLIP_GAIN) if name == "random" else (256,):
            want, clips = FR.convert(raw, fmt, g, L, M, taps)
            want = want[:want.size // BLK * BLK]
            assert want.size // BLK >= 3
            runs = [("one", tile), ("uneven", tile), ("each-4096", tile)] if full else [("each-4096", tile)]
            for cut, tl in runs + ([("uneven", SMALL_TILE)] if name == "random" or not full else []):
                got, got_clips = run_emulated(emu, raw, fmt, g, L, M, taps, cuts[cut], tl)
                assert got.size == want.size, (name, g, cut, tl)
                assert np.array_equal(got, want), (name, g, cut, tl, int(np.argmax(got != want)))
                assert got_clips == clips, (name, g, cut, tl)
            clip_seen += clips
    assert clip_seen > 0


@pytest.mark.parametrize("fin,d", RR.CORNERS, ids=RR.CORNER_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_corners_on_host_match_the_restatement(emu, wm, fmt, fin, d):
    check_design_on_the_emulator(emu, wm, fin, d, fmt)


def test_sampled_designs_on_host_match_the_restatement(emu, wm):
    """tests/resample_ref.py::sample_designs, one drawn format each (cu8 at gain x 1 goes through the kernel's cu8 entry point in
    test_resample_emulated.py); with WMBUS_RESAMPLE_FULL=1 cu8 as well, and the corners' whole matrix."""
    rng = np.random.default_rng(0x5A)
    for fin, d in RR.sample_designs():
        for fmt in ((FR.CU8,) if FULL else ()) + (WIDE[int(rng.integers(3))],):
            check_design_on_the_emulator(emu, wm, fin, d, fmt, full=FULL)


# (in_hz, decimation): T = 512 with the smallest tile, upsampling, the flagship ratio 25 / 32, integer decimation
LONG_STREAMS = [(25575000, 1), (1000000, 2), (2048000, 2), (3200000, 2), (2400000, 3)]


@pytest.mark.parametrize("fin,d", LONG_STREAMS, ids=[f"{f}-d{d}" for f, d in LONG_STREAMS])
def test_counters_beyond_32_bits(emu, wm, fin, d):
    """K0Args.n_first / in_first are 64-bit and nm = (n_first + t_first) M: a cs16 stream whose first 2^32 - (a push and a half) input
    samples were silence (x = 0: the carried history is zero, as in a fresh handle) is continued by 4096-byte pushes across 2^32
    input samples (at L > M the output counter is beyond 2^32 from the start).  in_first is a multiple of M, so n_first = in_first L / M
    is whole and no output is waiting for a block.  The restatement is evaluated at those output indices in Python integers.  At
    2.4 MS/s a live stream is there after half an hour; the HOST's counters (k0_plan in wm_api.hip) start at 0 and cannot be set
    through the ABI, so this reaches the kernel's arithmetic only."""
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    tile = emu.wm_emu_fmt_pick_tile(L, M, T)
    per_push = BLK // FR.BPS[FR.CS16]
    n_bytes = RR.blocks_input(L, M, FR.BPS[FR.CS16])
    n_push = n_bytes // BLK
    in_first = (2 ** 32 - per_push * (n_push // 2) - per_push // 2) // M * M
    n_first = in_first * L // M
    assert in_first < 2 ** 32 < in_first + n_bytes // 4 and in_first % M == 0 and n_first * M == in_first * L
    x = np.random.default_rng(fin).integers(-32768, 32768, (n_bytes // 4, 2))
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    n_end = ((in_first + x.shape[0]) * L + M - 1) // M
    idx = [((n * M) % L, (n * M) // L - in_first) for n in range(n_first, n_end)]      # phase, newest input within x: Python integers
    assert all(0 <= b < x.shape[0] for _, b in idx)
    p, b = np.array([i[0] for i in idx]), np.array([i[1] for i in idx]) + (T - 1)
    xx = np.concatenate([np.zeros((T - 1, 2), np.int64), x.astype(np.int64)])
    acc = np.zeros((len(idx), 2), np.int64)
    for k in range(T):
        acc += taps.astype(np.int64)[p, k][:, None] * xx[b - k]
    v = (acc * 256 + (128 << 30)) >> 30
    want = np.clip(v, 0, 255).astype(np.uint8).reshape(-1)
    want = want[:want.size // BLK * BLK]
    assert want.size // BLK >= 3
    for tl in (tile, SMALL_TILE):
        got, clips = run_emulated(emu, raw, FR.CS16, 256, L, M, taps, [BLK] * n_push, tl, start_at=(in_first, n_first))
        assert np.array_equal(got, want), (tl, int(np.argmax(got != want)) if got.size == want.size else (got.size, want.size))
        assert clips == int(np.count_nonzero((v < 0) | (v > 255)))
    # in_first L = n_first M: the phases repeat, so the very same samples at the start of a stream give the same bytes -- a check of
    # the Python-integer restatement above against format_ref.py, not of the kernel
    assert np.array_equal(want, FR.pipeline_bytes(raw, FR.CS16, 256, L, M, taps))


def test_gain_zero_is_unity_and_the_cu8_rule_is_unchanged(emu, wm):
    """input_gain_q8 = 0 means x 1; cu8 at x 1 through the resampler is byte for byte what tests/resample_ref.py defines."""
    raw = inputs(FR.CU8, N_BLOCKS * BLK)["random"]
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    want = RR.pipeline_bytes(raw, L, M, taps)
    assert np.array_equal(FR.pipeline_bytes(raw, FR.CU8, 256, L, M, taps), want)
    for g in (0, 256):
        assert np.array_equal(run_emulated(emu, raw, FR.CU8, g, L, M, taps, CUTS["uneven"], 190)[0], want)
        assert np.array_equal(run_emulated(emu, raw, FR.CU8, g, 1, 1, None, CUTS["uneven"], 72)[0], raw)


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_embedding_identity(wm, samples, fmt):
    """A cu8 byte u written as cs8 u - 128, cs16 128 (2u - 255) or cf32 (2u - 255) / 256 converts, at gain x 1, to the very bytes of the
    cu8 capture: u at a native rate, the bytes of tests/resample_ref.py behind the resampler.  Every cu8 golden tests the new paths."""
    rng = np.random.default_rng(99)
    for cu8 in (samples["samples2"][:64 * BLK], rng.integers(0, 256, 16 * BLK, dtype=np.uint8), np.arange(256, dtype=np.uint8).repeat(32)):
        raw = FR.embed(cu8, fmt)
        assert raw.size == cu8.size * FR.BPS[fmt] // 2
        y, clips = FR.convert(raw, fmt, 256)
        assert np.array_equal(y, cu8) and clips == 0
        assert np.array_equal(FR.pipeline_bytes(raw, fmt, 0), cu8[:cu8.size // BLK * BLK])
        for rate in (2048000, 2500000):
            L, M, T, taps = wm.resampler_design(rate, 1600000)
            assert np.array_equal(FR.pipeline_bytes(raw, fmt, 256, L, M, taps), RR.pipeline_bytes(cu8, L, M, taps)), rate


WEAK_SHIFT = 6


def weak_cs16(cu8):
    """A weak 16-bit capture: the cu8 capture embedded as cs16 and attenuated by an arithmetic shift of WEAK_SHIFT bits -- the
    generator's amplitude 60 (of 127.5) becomes 240 of 32768, its noise sigma 12."""
    return FR.raw_bytes(FR.embed(cu8, FR.CS16).view("<i2") >> WEAK_SHIFT, FR.CS16)


def test_gain_lets_a_weak_16_bit_capture_be_received(wm, oracle):
    """The synthetic 2.048 MS/s capture of test_resampled_capture_is_received_like_a_native_one (same seed, first N_YIELD frames) as a
    weak cs16 capture (6 bits down), through the restated resampler with a gain of 64 (input_gain_q8 = 64 * 256) and the oracle: at
    least the native 1.6 MS/s twin's yield minus 2 % of the frames placed, the margin of the cu8 resampler's test.  The same capture
    at gain x 1 is under one 8-bit step of signal and stays far outside that margin: the gain is what receives it.  (The shift of 6
    bits separates the two as it stands; 128 / 64 is a whole number, so this embedding loses no low bits to the shift.)"""
    raw, fr_raw, nat, fr_nat = yield_captures(wm)
    weak = weak_cs16(raw)
    assert np.abs(weak.view("<i2").astype(np.int64)).max() <= 2 * 255
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    opts = oracle.make_opts()
    y_gain, clips = FR.convert(weak, FR.CS16, 64 * 256, L, M, taps)
    got = received(fr_raw, oracle.run(y_gain[:y_gain.size // BLK * BLK], opts)["text"])
    unity = received(fr_raw, oracle.run(FR.pipeline_bytes(weak, FR.CS16, 256, L, M, taps), opts)["text"])
    ref = received(fr_nat, oracle.run(nat, opts)["text"])
    print(f"of the first {N_YIELD} frames placed: received weak cs16 at gain 64: {got}, at gain 1: {unity}, native cu8: {ref}; clipped {clips} of {y_gain.size}")
    assert got >= ref - 0.02 * N_YIELD
    assert unity < ref - 0.02 * N_YIELD
