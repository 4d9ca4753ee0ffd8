"""The frequency shift (cfg.input_shift_hz): the device source of the two K0-stage kernels with the rotation in their staging
(rtl-wmbus_amd/csrc/wm_k0_resample.h, k0_resample_block_t<FMT, true> and k0_convert_block<FMT, true>) on the coroutine block emulator
against the numpy restatement tests/shift_ref.py, byte for byte and clip count for clip count; a quarter-turn shift against integers
that never see the restatement; and a capture mixed up in double, brought back by the shift and read by the oracle.  No GPU needed."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import format_ref as FR
import shift_ref as SR
from test_formats_emulated import FMT_IDS, FORMATS, RATES, design, inputs
from test_resample_emulated import BLK, CUTS, N_BLOCKS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libshift_emu.so")
SRC = os.path.join(HERE, "emu", "shift_emu.cpp")
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))

OUT_HZ = 1600000                                    # decimation 2
RATE_IDS = [str(r) if r else "native" for r in RATES]
SHIFTS = [200000, -123457, 1, "-half"]              # "-half": -Fin / 2, the edge of the valid range
SHIFT_IDS = ["+200000", "-123457", "+1", "-half"]
GAINS = [256, 4096]


def fin_of(rate):
    return rate or OUT_HZ


def shift_of(rate, shift):
    return -(fin_of(rate) // 2) if shift == "-half" else shift


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_shift_new.restype = ctypes.c_void_p
    L.wm_emu_shift_new.argtypes = [ctypes.c_uint] * 5 + [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint32, ctypes.c_void_p]
    L.wm_emu_shift_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_shift_push.restype = ctypes.c_long
    L.wm_emu_shift_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_shift_pick_tile.restype = ctypes.c_uint
    L.wm_emu_shift_pick_tile.argtypes = [ctypes.c_uint] * 3
    L.wm_emu_shift_start_at.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    L.wm_emu_shift_convert_tile.restype = ctypes.c_uint
    L.wm_emu_shift_convert_tile.argtypes = [ctypes.c_uint]
    return L


def run_emulated(emu, wm, raw, fmt, gain, fin, f, L, M, taps, cuts, tile, start_at=None):
    """(the bytes the pipeline takes, push by push, concatenated; the clip counts of the pushes summed).  The step and the table are
    the library's (wmbus_shift_design).  start_at: (input samples, outputs) the stream already has behind it, all of them y = 0."""
    step, table = wm.shift_design(fin, f)
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_shift_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile, step, table.ctypes.data)
    if start_at is not None:
        emu.wm_emu_shift_start_at(h, start_at[0], start_at[1])
    got, off, clipped = [], 0, 0
    try:
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            win = np.full(BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M) + 64, 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            r = emu.wm_emu_shift_push(h, part.ctypes.data, part.size, win.ctypes.data, win.size - 64, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[-64:] == 0xA5)                 # nothing written past the window
            got.append(win[:r].copy()); clipped += clip.value
    finally:
        emu.wm_emu_shift_free(h)
    assert off == raw.size
    return np.concatenate(got), clipped


def library_tile(emu, wm, fmt, rate):
    """The tile wmbus_open picks for the path: the shift changes neither (the table lives in global memory, not in LDS)."""
    if rate == 0:
        return emu.wm_emu_shift_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, OUT_HZ)
    tile = emu.wm_emu_shift_pick_tile(L, M, T)
    assert tile > 0
    return tile


def shift_inputs(fmt, n_bytes):
    """inputs() of the format tests (random, minimum, maximum; cf32: wide and special values); cf32 also random BIT patterns; cs16
    also the four full-scale corners (+-32767 / -32768 in I and Q) in turn, where |y| = |x| sqrt 2 leaves int16 at every odd eighth
    of a turn."""
    named = dict(inputs(fmt, n_bytes))
    if fmt == FR.CF32:
        named["bits"] = np.random.default_rng(0xB175).integers(0, 256, n_bytes, dtype=np.uint8)
    if fmt == FR.CS16:
        corners = np.array([[32767, 32767], [-32768, 32767], [-32768, -32768], [32767, -32768]], np.int16)
        named["corners"] = FR.raw_bytes(np.resize(corners.repeat(5, axis=0), (n_bytes // 4, 2)).reshape(-1), fmt)
    return named


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fmt, rate, shift, cut):
    L, M, taps = design(wm, rate)
    fin, f = fin_of(rate), shift_of(rate, shift)
    tile = library_tile(emu, wm, fmt, rate)
    clip_seen = rot_clamps = 0
    for name, raw in shift_inputs(fmt, N_BLOCKS * BLK).items():
        rot_clamps += SR.rotation_clamps(raw, fmt, fin, f)
        for g in GAINS if name in ("random", "bits", "corners") else GAINS[:1]:
            want, clips = SR.convert(raw, fmt, fin, f, g, L, M, taps)
            want = want[:want.size // BLK * BLK]
            got, got_clips = run_emulated(emu, wm, raw, fmt, g, fin, f, L, M, taps, CUTS[cut], tile)
            assert got.size == want.size, (name, g)
            assert np.array_equal(got, want), (name, g, int(np.argmax(got != want)))
            assert got_clips == clips, (name, g)             # every output counted, the ones behind the last whole block too
            clip_seen += clips
    assert clip_seen > 0                                     # the output clamp is reached
    if fmt in (FR.CS16, FR.CF32) and shift in (200000, -123457):
        assert rot_clamps > 0                                # and the rotation's: full scale in I and Q, away from the axes
    if fmt in (FR.CU8, FR.CS8):
        assert rot_clamps == 0                               # 64 x 255 sqrt 2 < 32768


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_result_does_not_depend_on_the_tile(emu, wm, fmt, rate):
    """Small tiles: many blocks per push, block edges at every phase of the resampler and of the shift."""
    L, M, taps = design(wm, rate)
    fin = fin_of(rate)
    raw = shift_inputs(fmt, N_BLOCKS * BLK)["random"]
    tiles = (8, 72, 1000) if rate == 0 else (64, 190)
    for f in (200000, -123457):
        want, clips = SR.convert(raw, fmt, fin, f, 4096, L, M, taps)
        want = want[:want.size // BLK * BLK]
        for tile in tiles if f > 0 else tiles[1:]:           # the smallest tile is thousands of emulated blocks: once
            got, got_clips = run_emulated(emu, wm, raw, fmt, 4096, fin, f, L, M, taps, CUTS["uneven"], tile)
            assert np.array_equal(got, want) and got_clips == clips, (f, tile)


@pytest.mark.parametrize("rate", [0, 2500000], ids=["native", "2500000"])
def test_sample_counter_beyond_32_bits(emu, wm, rate):
    """The phase is (step m) mod 2^32 of the 64-bit stream index m = K0Args.in_first + index within the push: a cs16 stream whose
    first 2^32 - (ten and a half pushes) samples were silence (y = 0: the carried history is zero, as in a fresh handle) is continued
    by 4096-byte pushes across m = 2^32.  in_first is a multiple of M, so the resampler's phases start over and the restatement,
    with its table indices in Python integers from m0 on, describes the continuation."""
    L, M, taps = design(wm, rate)
    fin, f, fmt = fin_of(rate), -123457, FR.CS16
    per_push = BLK // FR.BPS[fmt]
    in_first = (2 ** 32 - 10 * per_push - per_push // 2) // M * M
    n_first = in_first * L // M
    assert n_first * M == in_first * L and in_first < 2 ** 32 < in_first + N_BLOCKS * per_push
    raw = shift_inputs(fmt, N_BLOCKS * BLK)["random"]
    want, clips = SR.convert(raw, fmt, fin, f, 4096, L, M, taps, m0=in_first)
    want = want[:want.size // BLK * BLK]
    assert not np.array_equal(want, SR.pipeline_bytes(raw, fmt, fin, f, 4096, L, M, taps))      # the start index matters
    for tile in (library_tile(emu, wm, fmt, rate), 72 if rate == 0 else 190):
        got, got_clips = run_emulated(emu, wm, raw, fmt, 4096, fin, f, L, M, taps, CUTS["each-4096"], tile, start_at=(in_first, n_first))
        assert np.array_equal(got, want) and got_clips == clips, tile


def test_a_quarter_turn_is_an_exact_multiplication_by_minus_j(emu, wm):
    """Not through the restatement: at f = Fin / 4 the step is 2^30, sample m uses table entry 256 (m mod 4) = (16384, 0), (0, 16384),
    (-16384, 0), (0, -16384), and (x 16384 + 8192) >> 14 = x.  A cs16 stream shifted by Fin / 4 at the native rate is therefore
    format_ref.convert of the stream times (-j)^m, worked out here in integers.  (-32768 is left out of the input: its negative is
    not an int16.)"""
    step, table = wm.shift_design(OUT_HZ, OUT_HZ // 4)
    assert step == 2 ** 30
    assert [table[256 * k].tolist() for k in range(4)] == [[16384, 0], [0, 16384], [-16384, 0], [0, -16384]]
    x = np.random.default_rng(0x14).integers(-32767, 32768, (N_BLOCKS * BLK // 4, 2))
    xi, xq = x[:, 0], x[:, 1]
    m = np.arange(x.shape[0]) % 4
    yi = np.select([m == 0, m == 1, m == 2, m == 3], [xi, xq, -xi, -xq])       # (xi + j xq) (-j)^m
    yq = np.select([m == 0, m == 1, m == 2, m == 3], [xq, -xi, -xq, xi])
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    turned = FR.raw_bytes(np.stack([yi, yq], axis=1).reshape(-1), FR.CS16)
    for g in (256, 4096):
        want, clips = FR.convert(turned, FR.CS16, g)
        want = want[:want.size // BLK * BLK]
        got, got_clips = run_emulated(emu, wm, raw, FR.CS16, g, OUT_HZ, OUT_HZ // 4, 1, 1, None, CUTS["uneven"], 72)
        assert np.array_equal(got, want) and got_clips == clips, g
    # and the other way round: -Fin / 4 multiplies by (+j)^m, which undoes it
    back, _ = run_emulated(emu, wm, turned, FR.CS16, 256, OUT_HZ, -(OUT_HZ // 4), 1, 1, None, CUTS["one"], 72)
    assert np.array_equal(back, FR.pipeline_bytes(raw, FR.CS16, 256))


GOLDEN_KEY = "rtlsdr_868.950M_1M6_samples2.cu8|"         # the default switches
PUSH = 128 * BLK


def emulate_capture(emu, wm, raw, fmt, gain, f):
    """A whole native-rate capture through the conversion kernel's emulation in pushes of PUSH raw bytes."""
    cuts = [PUSH] * (raw.size // PUSH) + ([raw.size % PUSH] if raw.size % PUSH else [])
    return run_emulated(emu, wm, raw, fmt, gain, OUT_HZ, f, 1, 1, None, cuts, emu.wm_emu_shift_convert_tile(fmt))


def fields(text, drop_rssi):
    """The lines' fields; MODE;CRC;3OF6;TS;RSSI;RSSI;ID;PAYLOAD -- without the two RSSI fields if asked."""
    rows = [ln.split(";") for ln in text.splitlines()]
    assert all(len(r) == 8 for r in rows)
    return [r[:4] + r[6:] if drop_rssi else r for r in rows]


@pytest.mark.parametrize("f", [200000, -123457], ids=["+200000", "-123457"])
def test_cs16_round_trip_gives_the_capture_back(emu, wm, oracle, samples, f):
    """samples2 mixed UP by f in double and written as cs16 at 90 counts per cu8 half-step; the shift by f with gain 364 / 256 gives
    back every byte of the original, none clipped, so the oracle prints the committed golden, RSSI fields included."""
    cu8 = samples["samples2"]
    assert cu8.size % BLK == 0
    raw = SR.round_trip_cs16(cu8, OUT_HZ, f)
    got, clips = emulate_capture(emu, wm, raw, FR.CS16, SR.CS16_ROUND_TRIP_GAIN, f)
    assert np.array_equal(got, cu8) and clips == 0
    want = BUNDLED[GOLDEN_KEY]
    assert len(want.splitlines()) == 4
    assert oracle.run(got, oracle.make_opts(show_algorithm=0))["text"] == want


@pytest.mark.parametrize("f", [200000, 50000], ids=["+200000", "+50000"])
def test_cu8_round_trip_is_within_one_count(emu, wm, oracle, samples, f):
    """The same through 8 bits: mixed up, scaled by 1 / 1.45 so that the rotated square fits, quantised to cu8.  The shift with gain
    371 / 256 is within one count of the original at every byte and the oracle reads the same four datagrams: mode, CRC flag, 3-of-6
    flag, identity and payload equal the golden's; the RSSI fields may differ."""
    cu8 = samples["samples2"]
    raw = SR.round_trip_cu8(cu8, OUT_HZ, f)
    got, _ = emulate_capture(emu, wm, raw, FR.CU8, SR.CU8_ROUND_TRIP_GAIN, f)
    assert got.size == cu8.size
    assert np.abs(got.astype(np.int64) - cu8.astype(np.int64)).max() <= 1
    assert np.array_equal(got, SR.pipeline_bytes(raw, FR.CU8, OUT_HZ, f, SR.CU8_ROUND_TRIP_GAIN))
    want = BUNDLED[GOLDEN_KEY]
    text = oracle.run(got, oracle.make_opts(show_algorithm=0))["text"]
    assert fields(text, True) == fields(want, True) and len(fields(want, True)) == 4
