"""The per-block AGC (cfg.input_agc): the ABI; the rule by hand; the device source of its kernels (rtl-wmbus_amd/csrc/wm_k0_resample.h:
k0_agc_gain_block and the AG instantiations of k0_resample_block_t / k0_convert_block) on the coroutine block emulator against the numpy
restatement tests/agc_ref.py, byte for byte, clip count for clip count and gain for gain; and what the AGC is for, through the oracle:
weak captures and captures of mixed level, which no fixed gain serves.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import agc_ref as AR
import dc_ref as DR
import format_ref as FR
from test_dc_emulated import OUT_HZ, RATE_IDS, RATES, dc_inputs
from test_formats_emulated import FMT_IDS, FORMATS, design
from test_resample_emulated import BLK, CUTS, N_BLOCKS, received

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libagc_emu.so")
SRC = os.path.join(HERE, "emu", "agc_emu.cpp")

assert RATES == [0, 2048000, 2500000]               # native (the conversion kernel), and two rates through the resampler to 1.6 MS/s
RS = [0, 6]                                         # without and with the DC blocker in front
SHIFTS = [0, 250000]
IGNORED_GAIN = 12345                                # K0Args.gain_q8 as the emulator passes it: an AG stage must not look at it
JUMP = 75                                           # the level ratio of the jump input (37.5 dB)


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here, the restated yields included, describes cfg.input_agc: on a library without the field no test of this file says
    anything, so none passes."""
    assert "input_agc" in [f[0] for f in wm.Cfg._fields_] and "wmbus_read_input_gain" in wm.EXPORTS


def test_the_abi_has_the_agc_field(wm):
    """Fails on a tree without the feature.  The field sits directly in front of clock_waves: an existing test pins the seven fields
    from clock_waves on."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_agc")
    assert names[k - 1] == "k1_tiles_per_block" and names[k + 1] == "clock_waves"
    assert names[k + 1:] == ["clock_waves", "line_levels", "input_rate_hz", "input_shift_hz", "input_dc", "input_format", "input_gain_q8"]
    assert dict((f[0], f[1]) for f in wm.Cfg._fields_)["input_agc"] is ctypes.c_uint
    assert [f[0] for f in wm.Timing._fields_][-2:] == ["input_bytes_out", "input_clipped"]      # wmbus_timing did not change
    c = wm.Cfg()
    c.input_agc = 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_agc == 0
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_agc;", "long wmbus_read_input_gain(wmbus_ctx *ctx, unsigned stream, uint16_t *g, size_t cap);",
                 "g[k] = clamp(floor((96 << U) / max(P[k], 1)), 1, 65535)"):
        assert word in hdr, word
    assert hdr.index("unsigned k1_tiles_per_block;") < hdr.index("unsigned input_agc;") < hdr.index("unsigned clock_waves;")
    assert "wmbus_read_input_gain" in wm.EXPORTS and hasattr(wm.lib(), "wmbus_read_input_gain")
    assert hasattr(wm.Receiver, "read_input_gain")
    assert wm._make_cfg(input_agc=1).input_agc == 1 and wm._make_cfg().input_agc == 0


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_agc_new.restype = ctypes.c_void_p
    L.wm_emu_agc_new.argtypes = [ctypes.c_uint] * 5 + [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint]
    L.wm_emu_agc_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_agc_push.restype = ctypes.c_long
    L.wm_emu_agc_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_agc_read.restype = ctypes.c_long
    L.wm_emu_agc_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.wm_emu_agc_pick_tile.restype = ctypes.c_uint
    L.wm_emu_agc_pick_tile.argtypes = [ctypes.c_uint] * 3
    L.wm_emu_agc_convert_tile.restype = ctypes.c_uint
    L.wm_emu_agc_convert_tile.argtypes = [ctypes.c_uint]
    return L


def run_emulated(emu, wm, raw, fmt, R, fin, f, L, M, taps, cuts, tile):
    """(the bytes the pipeline takes, push by push, concatenated; the clip counts of the pushes summed; the gain of every level block,
    int64 [n], read push by push as wmbus_read_input_gain reads it).  R = 0: no blocker; f = 0: no shift."""
    step, table = wm.shift_design(fin, f) if f else (0, None)
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_agc_new(fmt, IGNORED_GAIN, L, M, T, tp.ctypes.data if tp is not None else None, tile, step, table.ctypes.data if f else None, R)
    got, gains, off, clipped = [], [], 0, 0
    try:
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            win = np.full(BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M) + 64, 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            r = emu.wm_emu_agc_push(h, part.ctypes.data, part.size, win.ctypes.data, win.size - 64, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[-64:] == 0xA5)                 # nothing written past the window
            got.append(win[:r].copy()); clipped += clip.value
            n_blk = n // FR.BPS[fmt] // AR.BLOCK
            g = np.full(n_blk + 1, 0x7777, np.uint16)
            assert emu.wm_emu_agc_read(h, g.ctypes.data, n_blk + 1) == n_blk
            assert g[n_blk] == 0x7777
            gains.append(g[:n_blk].astype(np.int64))
    finally:
        emu.wm_emu_agc_free(h)
    assert off == raw.size
    return np.concatenate(got), clipped, np.concatenate(gains)


def library_tile(emu, wm, fmt, rate):
    """The tile wmbus_open picks for the path: the AGC changes neither (the table lives in global memory)."""
    if rate == 0:
        return emu.wm_emu_agc_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, OUT_HZ)
    tile = emu.wm_emu_agc_pick_tile(L, M, T)
    assert tile > 0
    return tile


# per format: (centre, the weak level's amplitude; the strong one is JUMP times it), in the format's own units
LEVELS = {FR.CU8: (128, 1), FR.CS8: (0, 1), FR.CS16: (0, 400), FR.CF32: (0.0, 0.012)}


def jump_input(fmt, n_bytes):
    """Noise whose level jumps UP by a factor of 75 at a sample that is neither a level-block nor a push boundary of any cut, and back
    DOWN at another one (behind the resampler the outputs behind that edge hold strong samples under the weak block's gain)."""
    rng = np.random.default_rng(0xA6C + fmt)
    n = n_bytes // FR.BPS[fmt]
    mid, amp = LEVELS[fmt]
    up, down = 3 * (BLK // FR.BPS[fmt]) + 777, 9 * (BLK // FR.BPS[fmt]) + 1301
    for at in (up, down):
        assert at % AR.BLOCK and (at * FR.BPS[fmt]) % BLK and at < n
    m = np.arange(n)[:, None]
    a = np.where((m >= up) & (m < down), JUMP * amp, amp)
    if fmt == FR.CF32:
        return FR.raw_bytes((mid + a * rng.uniform(-1.0, 1.0, (n, 2))).reshape(-1), fmt)
    return FR.raw_bytes((mid + rng.integers(-1, 2, (n, 2)) * rng.integers(0, np.broadcast_to(a + 1, (n, 2)))).reshape(-1), fmt)


def test_rule_by_hand():
    """g = clamp(floor((96 << U) / max(P, 1)), 1, 65535), U = 9 for the 8-bit formats and 16 for cs16 / cf32, worked out on paper:
    P = 0 and P = 1: 96 << 16 = 6291456 is above the clamp, 96 << 9 = 49152 is not; cu8 P = 510 (both bytes 0 or 255): 49152 / 510 =
    96.4; cs16 P = 370: 6291456 = 370 x 17003 + 346; cs16 P = 65536 (both -32768): exactly 96; the two sides of the upper clamp:
    6291456 / 96 = 65536 -> 65535 and 6291456 = 97 x 64860 + 36.  (The issue that asked for this test quotes 17004 and 64863 for P = 370
    and P = 97; those are not what its own rule gives -- 370 x 17004 and 97 x 64863 both lie above 96 << 16 -- and the rule is the contract.)"""
    for P in (0, 1):
        assert AR.gain_of(P, FR.CS16) == 65535 and AR.gain_of(P, FR.CF32) == 65535
        assert AR.gain_of(P, FR.CU8) == 49152 and AR.gain_of(P, FR.CS8) == 49152
    assert AR.gain_of(510, FR.CU8) == 96
    assert AR.gain_of(370, FR.CS16) == 17003 and 370 * 17003 <= 96 << 16 < 370 * 17004
    assert AR.gain_of(65536, FR.CS16) == 96
    assert AR.gain_of(96, FR.CS16) == 65535 and AR.gain_of(97, FR.CS16) == 64860 and 97 * 64860 <= 96 << 16 < 97 * 64861
    x = np.zeros((2 * AR.BLOCK, 2), np.int64)
    x[5] = (300, -70)
    x[AR.BLOCK + 9] = (-32768, -32768)
    assert AR.block_gain(x, FR.CS16).tolist() == [17003, 96]
    # the peak lands on 96: all-128 cu8 is x = 1, P = 2, g = 24576, byte 128 + (16384 * 24576 >> 23) = 176; the strongest cu8 byte
    # pair (0, 255) is x = -+255, P = 510, g = 96: 128 + floor(-255 * 96 / 512) = 80 and 128 + floor(255 * 96 / 512) = 175
    y, clips, g = AR.convert(np.full(2 * AR.BLOCK, 128, np.uint8), FR.CU8)
    assert g.tolist() == [24576] and np.all(y == 176) and clips == 0
    y, clips, g = AR.convert(np.tile(np.array([0, 255], np.uint8), AR.BLOCK), FR.CU8)
    assert g.tolist() == [96] and y[:2].tolist() == [80, 175] and clips == 0


def test_kernels_follow_the_rule_worked_out_by_hand(emu, wm):
    """The same numbers through the device source, not through the restatement: eight cs16 level blocks whose peaks are 0, 1, 370, 65536,
    96, 97, 370 again (as (0, -370): the peak is |I| + |Q|, not a component) and 192; then cu8 blocks of P = 510 and of silence."""
    peaks = [(0, 0), (0, 1), (300, -70), (-32768, -32768), (96, 0), (-97, 0), (0, -370), (-100, 92)]
    x = np.zeros((len(peaks) * AR.BLOCK, 2), np.int64)
    for k, p in enumerate(peaks):
        x[k * AR.BLOCK + 37 * k + 11] = p                    # one sample of the block, in another lane's load each time
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    y, clips, g = run_emulated(emu, wm, raw, FR.CS16, 0, OUT_HZ, 0, 1, 1, None, [BLK, 3 * BLK], 72)
    assert g.tolist() == [65535, 65535, 17003, 96, 65535, 64860, 17003, 32768]
    k = 2 * AR.BLOCK + 37 * 2 + 11                           # (300, -70) x 17003 / 65536 = 77.8, -18.2: floors
    assert y[2 * k:2 * k + 2].tolist() == [128 + 77, 128 - 19] and clips == 0
    k = 3 * AR.BLOCK + 37 * 3 + 11                           # full scale lands on 128 - 48 = 80 in both components
    assert y[2 * k:2 * k + 2].tolist() == [80, 80]
    cu8 = np.concatenate([np.tile(np.array([0, 255], np.uint8), AR.BLOCK), np.full(2 * 7 * AR.BLOCK, 128, np.uint8)])
    y, clips, g = run_emulated(emu, wm, cu8, FR.CU8, 0, OUT_HZ, 0, 1, 1, None, [BLK, BLK], 72)
    assert g.tolist() == [96] + [24576] * 7 and clips == 0
    assert y[:2].tolist() == [80, 175] and np.all(y[2 * AR.BLOCK:] == 176)


def check(emu, wm, raw, fmt, R, rate, f, cut, tile, tag):
    L, M, taps = design(wm, rate)
    fin = rate or OUT_HZ
    want, clips, g = AR.convert(raw, fmt, R, fin, f, L, M, taps)
    want = want[:want.size // BLK * BLK]
    got, got_clips, got_g = run_emulated(emu, wm, raw, fmt, R, fin, f, L, M, taps, CUTS[cut], tile)
    assert np.array_equal(got_g, g), (tag, int(np.argmax(got_g != g)))
    assert got.size == want.size, tag
    assert np.array_equal(got, want), (tag, int(np.argmax(got != want)))
    assert got_clips == clips, tag                       # every output counted, the ones behind the last whole block too
    return want, clips, g


@pytest.mark.parametrize("f", SHIFTS, ids=["noshift", "+250000"])
@pytest.mark.parametrize("R", RS, ids=[f"R{r}" for r in RS])
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fmt, rate, R, f):
    """The inputs of the blocker's test under the 4096-byte pushes and the jump input under all three cuts."""
    tile = library_tile(emu, wm, fmt, rate)
    for name, raw in dc_inputs(fmt, N_BLOCKS * BLK).items():
        want, clips, g = check(emu, wm, raw, fmt, R, rate, f, "each-4096", tile, (name, "each-4096"))
        if name in ("min", "max") and R:                     # the blocker takes all of it: x' = 0, P = 0, the gain at its clamp, mid-scale
            assert np.all(want == 128) and clips == 0 and np.all(g == AR.gain_of(0, fmt))
    raw = jump_input(fmt, N_BLOCKS * BLK)
    gains = set()
    for cut in CUTS:
        want, clips, g = check(emu, wm, raw, fmt, R, rate, f, cut, tile, ("jump", cut))
        gains.add(tuple(g.tolist()))
    assert len(gains) == 1                                   # the gains do not depend on the cut
    assert g.max() >= 30 * g.min()                           # both levels are in the input (the 8-bit formats' x is odd: P = 6 against 302, not 1 : 75)
    if rate == 0:
        assert clips == 0                                    # at the native rate |component| <= P: nothing can clip


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_result_does_not_depend_on_the_tile(emu, wm, fmt, rate):
    """Small odd tiles: many blocks per push, block edges inside level blocks and at every phase of the resampler."""
    raw = jump_input(fmt, N_BLOCKS * BLK)
    tiles = (8, 72, 1000) if rate == 0 else (64, 190)
    for f in SHIFTS:
        for tile in tiles if f == 0 else tiles[1:]:          # the smallest tile is thousands of emulated blocks: once
            check(emu, wm, raw, fmt, 6 if f else 0, rate, f, "uneven", tile, (f, tile))


def test_behind_the_resampler_a_strong_to_weak_edge_may_clip_and_is_counted(emu, wm):
    """The documented consequence, on the restatement and on the device source: full-scale cs16 followed by weak cs16 at 2.048 MS/s.  The
    outputs whose newest input lies in the first weak block still sum strong samples, under the weak block's gain."""
    n = 8 * AR.BLOCK
    rng = np.random.default_rng(9)
    x = rng.integers(-1, 2, (n, 2)) * np.where(np.arange(n)[:, None] < 4 * AR.BLOCK, 30000, 40)
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    L, M, taps = design(wm, 2048000)
    want, clips, g = AR.convert(raw, FR.CS16, 0, 2048000, 0, L, M, taps)
    assert 0 < clips <= 2 * taps.shape[1] * L // M + 2       # only outputs that reach back across the edge: T input samples' worth
    got, got_clips, got_g = run_emulated(emu, wm, raw, FR.CS16, 0, 2048000, 0, L, M, taps, [BLK, 3 * BLK], library_tile(emu, wm, FR.CS16, 2048000))
    assert got_clips == clips and np.array_equal(got_g, g) and np.array_equal(got, want[:got.size])


# ---- what the AGC is for: yields through the oracle --------------------------------------------------------------------------------

KINDS = 1 | 2 | 4 | 8                                # T1 | C1A | C1B | S1
FIXED = [1, 16, 64, 128]                             # the fixed gains the mix is held against, linear


def capture_a(wm, fs_khz=1600, n=6400000):
    """Weak-to-medium traffic: 100 frames/s, amplitude 20 cu8 steps, noise sigma 3."""
    return wm.synth_capture(seed=77, n_samples=n, fs_khz=fs_khz, kinds=KINDS, frames_per_s=100.0, amplitude=20.0, noise_sigma=3.0)


def capture_b(wm, fs_khz=1600, n=6400000):
    """A few strong telegrams: 15 frames/s, amplitude 100, no noise."""
    return wm.synth_capture(seed=78, n_samples=n, fs_khz=fs_khz, kinds=KINDS, frames_per_s=15.0, amplitude=100.0, noise_sigma=0.0)


def x_of(cu8):
    return 2 * np.asarray(cu8, np.uint8).astype(np.int64) - 255


def run(oracle, frames, y):
    return received(frames, oracle.run(np.ascontiguousarray(y[:y.size // BLK * BLK]), oracle.make_opts())["text"])


def test_agc_receives_a_weak_cs16_capture_that_gain_1_loses(wm, oracle):
    """Capture A written as cs16 = 4 (2u - 255): a 160-count amplitude of 32768, what a 16-bit receiver with its gain set low delivers.
    bar = the clean capture's yield minus 2 % of the frames placed (the margin of the existing yield tests).  Measured: 188 placed, 187
    clean, 187 with the AGC, 0 at gain x 1 (187 at the best fixed gain, x 64); as cf32 = (2u - 255) / 8192 the same."""
    cu8, frames = capture_a(wm)
    placed = len(frames)
    assert placed >= 150
    clean = run(oracle, frames, cu8)
    bar = clean - 0.02 * placed
    cs16 = FR.raw_bytes(4 * x_of(cu8), FR.CS16)
    y, clips, g = AR.convert(cs16, FR.CS16)
    agc = run(oracle, frames, y)
    plain = run(oracle, frames, FR.convert(cs16, FR.CS16, 256)[0])
    cf32 = FR.raw_bytes((x_of(cu8) / 8192.0).astype(np.float32), FR.CF32)
    agc_f = run(oracle, frames, AR.convert(cf32, FR.CF32)[0])
    plain_f = run(oracle, frames, FR.convert(cf32, FR.CF32, 256)[0])
    print(f"of {placed} frames placed: clean {clean}; cs16 with input_agc {agc} (g {g.min()} ... {g.max()}, clipped {clips}), gain x 1 {plain}; "
          f"cf32 with input_agc {agc_f}, gain x 1 {plain_f}")
    assert agc >= bar and plain < bar
    assert agc_f >= bar and plain_f < bar


def test_agc_and_blocker_together_receive_a_weak_offset_capture(wm, oracle):
    """An amplitude-5 cu8 capture (seed 79, noise sigma 1) written as cs8 with an I/Q offset of (+12, -9): the blocker alone leaves a
    signal too weak for the reference's chain, the AGC alone levels the offset, not the signal.  Bars counted against the frames placed:
    input_dc = 6 plus the AGC receive at least 98 %, the other three stay below that.  Measured: 177 placed; 177, and 0, 0, 0."""
    cu8, frames = wm.synth_capture(seed=79, n_samples=6400000, fs_khz=1600, kinds=KINDS, frames_per_s=100.0, amplitude=5.0, noise_sigma=1.0)
    placed = len(frames)
    assert placed >= 150
    cs8 = FR.raw_bytes(DR.add_offset_cu8(cu8, 12, -9).astype(np.int64) - 128, FR.CS8)
    both = run(oracle, frames, AR.convert(cs8, FR.CS8, 6)[0])
    untouched = run(oracle, frames, FR.convert(cs8, FR.CS8, 256)[0])
    blocker = run(oracle, frames, DR.convert(cs8, FR.CS8, 6)[0])
    agc = run(oracle, frames, AR.convert(cs8, FR.CS8)[0])
    print(f"of {placed} frames placed: input_dc = 6 plus input_agc {both}; untouched {untouched}, the blocker alone {blocker}, the AGC alone {agc}")
    bar = 0.98 * placed
    assert both >= bar
    assert untouched == 0
    assert blocker < bar and agc < bar


def test_agc_serves_a_mix_of_levels_that_no_fixed_gain_serves(wm, oracle):
    """Weak traffic A plus strong telegrams B, 37 dB apart, as cs16 = clip(4 xA + 60 xB).  Counted against the frames placed: the AGC's
    strong count is at least every fixed gain's, its weak count at least the best fixed weak count minus 2 % of the weak frames placed,
    and every fixed gain in x 1, 16, 64, 128 falls below one of the two bars (strong: the AGC's count minus 2 % of the strong frames
    placed).  Measured: 109 weak and 56 strong with the AGC, no byte clipped; x 1 and x 16: 0 weak; x 64 and x 128: 110 weak, 51 and 52
    strong.  The 2.048 MS/s variants are printed; of them only the weak capture is held to a bar."""
    a, frames_a = capture_a(wm)
    b, frames_b = capture_b(wm)
    mix = FR.raw_bytes(np.clip(4 * x_of(a) + 60 * x_of(b), -32768, 32767), FR.CS16)
    y, clips, g = AR.convert(mix, FR.CS16)
    weak, strong = run(oracle, frames_a, y), run(oracle, frames_b, y)
    print(f"mix: {len(frames_a)} weak and {len(frames_b)} strong frames placed; input_agc {weak} weak, {strong} strong (g {g.min()} ... {g.max()}, clipped {clips})")
    fixed = {}
    for k in FIXED:
        yk, ck = FR.convert(mix, FR.CS16, 256 * k)
        fixed[k] = (run(oracle, frames_a, yk), run(oracle, frames_b, yk))
        print(f"mix: gain x {k}: {fixed[k][0]} weak, {fixed[k][1]} strong, clipped {ck}")
    weak_bar = max(v[0] for v in fixed.values()) - 0.02 * len(frames_a)
    strong_bar = strong - 0.02 * len(frames_b)
    assert strong >= max(v[1] for v in fixed.values())
    assert weak >= weak_bar
    for k, (w, s) in fixed.items():
        assert w < weak_bar or s < strong_bar, k

    # behind the 2.048 MS/s resampler; captures synthesised at that rate (other frames than above: the generator's one random sequence)
    L, M, taps = design(wm, 2048000)
    a2, frames_a2 = capture_a(wm, 2048, 8192000)
    b2, frames_b2 = capture_b(wm, 2048, 8192000)
    weak16 = FR.raw_bytes(4 * x_of(a2), FR.CS16)
    y, clips, g = AR.convert(weak16, FR.CS16, 0, 2048000, 0, L, M, taps)
    agc2 = run(oracle, frames_a2, y)
    best2 = run(oracle, frames_a2, FR.convert(weak16, FR.CS16, 256 * 64, L, M, taps)[0])
    print(f"2.048 MS/s, weak: {len(frames_a2)} placed; input_agc {agc2} (clipped {clips} of {y.size}), gain x 64 {best2}")
    mix2 = FR.raw_bytes(np.clip(4 * x_of(a2) + 60 * x_of(b2), -32768, 32767), FR.CS16)
    y, clips, g = AR.convert(mix2, FR.CS16, 0, 2048000, 0, L, M, taps)
    y64 = FR.convert(mix2, FR.CS16, 256 * 64, L, M, taps)[0]
    print(f"2.048 MS/s, mix: {len(frames_a2)} weak and {len(frames_b2)} strong placed; input_agc {run(oracle, frames_a2, y)} weak, {run(oracle, frames_b2, y)} strong "
          f"(clipped {clips}); gain x 64 {run(oracle, frames_a2, y64)} weak, {run(oracle, frames_b2, y64)} strong")
    assert agc2 >= best2 - 0.02 * len(frames_a2)
