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
    L.wm_emu_fmt_convert_tile.restype = ctypes.c_uint
    L.wm_emu_fmt_convert_tile.argtypes = [ctypes.c_uint]
    return L


def design(wm, rate):
    """(L, M, taps) of the path `rate` takes at decimation 2; taps None: the conversion kernel."""
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, 1600000)
    return L, M, taps


def run_emulated(emu, raw, fmt, gain, L, M, taps, cuts, tile):
    """(the bytes the pipeline takes, push by push, concatenated; the clip counts of the pushes summed)."""
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_fmt_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile)
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
