"""The I/Q DC blocker (cfg.input_dc): the ABI; the recurrence by hand; the device source of its three kernels
(rtl-wmbus_amd/csrc/wm_k0_resample.h: k0_dc_sums_block, k0_dc_plan_block and the DC instantiations of k0_resample_block_t /
k0_convert_block) on the coroutine block emulator against the numpy restatement tests/dc_ref.py, byte for byte, clip count for clip
count and dc for dc; and what the blocker is for, through the oracle: a capture with an I/Q offset smaller than its signal, which the
reference's chain loses and the blocker gives back.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dc_ref as DR
import format_ref as FR
from test_formats_emulated import CF32_ROW, FMT_IDS, FORMATS, design
from test_resample_emulated import BLK, CUTS, N_BLOCKS, received

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libdc_emu.so")
SRC = os.path.join(HERE, "emu", "dc_emu.cpp")

OUT_HZ = 1600000                                    # decimation 2
RATES = [0, 2048000, 2500000]                       # 0: already at 1.6 MS/s, the conversion kernel; else the resampler to 1.6 MS/s
RATE_IDS = [str(r) if r else "native" for r in RATES]
RS = [1, 6, 12]
SHIFTS = [0, 250000]
CLIP_GAIN = 4096                                    # x 16: random full-range input clips


def test_the_abi_has_the_dc_field(wm):
    """Fails on a tree without the feature.  The field sits between input_shift_hz and input_format: existing tests pin
    input_shift_hz right behind input_rate_hz and input_format, input_gain_q8 as the last two."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_dc")
    assert names[k - 1] == "input_shift_hz" and names[k + 1:] == ["input_format", "input_gain_q8"]
    assert dict((f[0], f[1]) for f in wm.Cfg._fields_)["input_dc"] is ctypes.c_uint
    assert [f[0] for f in wm.Timing._fields_][-2:] == ["input_bytes_out", "input_clipped"]      # wmbus_timing did not change
    c = wm.Cfg()
    c.input_dc = 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_dc == 0
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_dc;", "long wmbus_read_input_dc(wmbus_ctx *ctx, unsigned stream, int16_t *iq, size_t cap_pairs);"):
        assert word in hdr, word
    assert hdr.index("int input_shift_hz;") < hdr.index("unsigned input_dc;") < hdr.index("unsigned input_format;")
    assert "wmbus_read_input_dc" in wm.EXPORTS and hasattr(wm.lib(), "wmbus_read_input_dc")
    assert hasattr(wm.Receiver, "read_input_dc")


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_dc_new.restype = ctypes.c_void_p
    L.wm_emu_dc_new.argtypes = [ctypes.c_uint] * 5 + [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint]
    L.wm_emu_dc_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_dc_push.restype = ctypes.c_long
    L.wm_emu_dc_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_dc_read.restype = ctypes.c_long
    L.wm_emu_dc_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.wm_emu_dc_pick_tile.restype = ctypes.c_uint
    L.wm_emu_dc_pick_tile.argtypes = [ctypes.c_uint] * 3
    L.wm_emu_dc_convert_tile.restype = ctypes.c_uint
    L.wm_emu_dc_convert_tile.argtypes = [ctypes.c_uint]
    return L


def run_emulated(emu, wm, raw, fmt, R, gain, fin, f, L, M, taps, cuts, tile):
    """(the bytes the pipeline takes, push by push, concatenated; the clip counts of the pushes summed; the dc of every level block,
    int64 [n, 2], read push by push as wmbus_read_input_dc reads it).  f = 0: no shift (the SH = false instantiations)."""
    step, table = wm.shift_design(fin, f) if f else (0, None)
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_dc_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile, step, table.ctypes.data if f else None, R)
    got, dcs, off, clipped = [], [], 0, 0
    try:
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            win = np.full(BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M) + 64, 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            r = emu.wm_emu_dc_push(h, part.ctypes.data, part.size, win.ctypes.data, win.size - 64, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[-64:] == 0xA5)                 # nothing written past the window
            got.append(win[:r].copy()); clipped += clip.value
            n_blk = n // FR.BPS[fmt] // DR.BLOCK
            dc = np.full((n_blk + 1, 2), 0x7777, np.int16)
            assert emu.wm_emu_dc_read(h, dc.ctypes.data, n_blk + 1) == n_blk
            dcs.append(dc[:n_blk].astype(np.int64))
    finally:
        emu.wm_emu_dc_free(h)
    assert off == raw.size
    return np.concatenate(got), clipped, np.concatenate(dcs)


def library_tile(emu, wm, fmt, rate):
    """The tile wmbus_open picks for the path: the blocker changes neither (the table lives in global memory)."""
    if rate == 0:
        return emu.wm_emu_dc_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, OUT_HZ)
    tile = emu.wm_emu_dc_pick_tile(L, M, T)
    assert tile > 0
    return tile


# per format: (lowest value, highest value, the offsets of the inputs below in the format's own units, noise amplitude of "step")
RANGE = {FR.CU8: (0, 255, (12, -9), (-40, 60), 10), FR.CS8: (-128, 127, (12, -9), (-40, 60), 10),
         FR.CS16: (-32768, 32767, (1536, -1152), (-30000, 30000), 5000), FR.CF32: (-1.0, 1.0, (12 / 256, -9 / 256), (-0.9, 0.9), 0.15)}


def dc_inputs(fmt, n_bytes):
    """Raw byte streams of n_bytes.  offset: random over the format's full range plus a constant (I, Q) offset, clipped to the range;
    min / max: all-minimum, all-maximum (the blocker takes all of it: x' = 0); step: noise around an offset that jumps to another, far
    one at a sample that is neither a level-block nor a push boundary of any cut (the far one saturates x - dc in the 16-bit formats);
    cf32 also the row of special values and random BIT patterns."""
    rng = np.random.default_rng(0xDC0 + fmt)
    n = n_bytes // FR.BPS[fmt]                           # IQ samples
    lo, hi, off, far, amp = RANGE[fmt]
    whole = fmt != FR.CF32

    def draw(a, b):
        return rng.integers(a, b + 1, (n, 2)).astype(np.float64) if whole else rng.uniform(a, b, (n, 2))

    def enc(v):
        v = np.clip(v, lo, hi)
        return FR.raw_bytes((np.rint(v) if whole else v).reshape(-1), fmt)
    at = 3 * (BLK // FR.BPS[fmt]) + 777                  # inside the second push of the uneven cut, inside a level block
    assert at % DR.BLOCK and (at * FR.BPS[fmt]) % BLK
    step = draw(-amp, amp) + np.where(np.arange(n)[:, None] < at, np.array(off)[None, :], np.array(far)[None, :])
    named = {"offset": enc(draw(lo, hi) + np.array(off)[None, :]), "min": enc(np.full((n, 2), lo)), "max": enc(np.full((n, 2), hi)), "step": enc(step)}
    if fmt == FR.CF32:
        named["special"] = FR.raw_bytes(np.resize(CF32_ROW, 2 * n), fmt)
        named["bits"] = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    return named


def test_recurrence_by_hand():
    """A[0] = S[0] << R, A[k] = A[k-1] - (A[k-1] >> R) + S[k], dc = (A + 2^(8+R)) >> (9+R), worked out on paper.
    R = 1, S = -1, -2, -511: A = -2, -2 + 1 - 2 = -3, -3 - (-3 >> 1 = -2) - 511 = -512 and dc = (0) >> 10 = 0; a >> that truncated
    (-3 / 2 = -1) would give A = -513 and dc = -1.
    R = 1, S = 1024, -1024, -3, -1, -2000: A = 2048, 0, -3, -2, -2001; dc = 2560 >> 10 = 2, 0, 0, 0, -1489 >> 10 = -2.
    R = 12, S = 51200 (x = 100 throughout), 0, 0: A = 51200 * 4096, * 4095 / 4096 each step (minus the floor): dc stays 100 for the
    first steps of a time constant of 4096 blocks.
    The clamp: S = -2^24 (every x = -32768) gives dc = -32768 at any R; S = 2^24 - 512 (every x = 32767) gives 32767."""
    assert DR.recurrence([-1, -2, -511], 1) == [0, 0, 0]
    assert DR.recurrence([1024, -1024, -3, -1, -2000], 1) == [2, 0, 0, 0, -2]
    assert DR.recurrence([51200, 0, 0], 12) == [100, 100, 100]
    assert DR.recurrence([51200] + [0] * 5000, 12)[-1] < 40            # e^-1.22 of 100 after 5000 of 4096 blocks
    for R in (1, 6, 12):
        assert DR.recurrence([-(1 << 24)] * 3, R) == [-32768] * 3 and DR.recurrence([(1 << 24) - 512] * 3, R) == [32767] * 3
    x = np.zeros((3 * DR.BLOCK, 2), np.int64)
    x[0, 0], x[DR.BLOCK:DR.BLOCK + 2, 0], x[2 * DR.BLOCK:2 * DR.BLOCK + 511, 0] = -1, -1, -1
    x[:, 1] = 7
    y, dc = DR.block_dc(x, 1)
    assert dc.tolist() == [[0, 7], [0, 7], [0, 7]] and np.array_equal(y[:, 0], x[:, 0]) and np.all(y[:, 1] == 0)
    # x' saturates: full scale one way, then the other, at R = 12.  I: A1 / 2^21 = 32767 * 4095 / 4096 - 8 = 32751.0002, + 1/2, floor;
    # Q: -32768 * 4095 / 4096 + 7.9998 = -32752.0002, + 1/2, floor = -32752
    y, dc = DR.block_dc(np.array([[32767, -32768]] * DR.BLOCK + [[-32768, 32767]] * DR.BLOCK), 12)
    assert dc.tolist() == [[32767, -32768], [32751, -32752]]
    assert y[0].tolist() == [0, 0] and y[-1].tolist() == [-32768, 32767]


def test_kernels_follow_the_recurrence_worked_out_by_hand(emu, wm):
    """The same numbers through the device source, not through the restatement: cs16 level blocks whose sums are -1, -2, -511 in I (the
    floor of a negative A) and 51200 = 512 x 100 in Q, at R = 1; and Q again at R = 12 over blocks of 100, 0, 0."""
    n = 8 * DR.BLOCK                                     # two 4096-byte cs16 pushes of four level blocks
    x = np.zeros((n, 2), np.int64)
    x[0, 0], x[DR.BLOCK:DR.BLOCK + 2, 0], x[2 * DR.BLOCK:2 * DR.BLOCK + 511, 0] = -1, -1, -1
    x[:, 1] = 100
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    _, _, dc = run_emulated(emu, wm, raw, FR.CS16, 1, 256, OUT_HZ, 0, 1, 1, None, [2 * BLK, 2 * BLK], 72)
    assert dc[:3, 0].tolist() == [0, 0, 0] and np.all(dc[:, 1] == 100)
    x[DR.BLOCK:, 1] = 0
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    _, _, dc = run_emulated(emu, wm, raw, FR.CS16, 12, 256, OUT_HZ, 0, 1, 1, None, [BLK] * 4, 72)
    assert dc[:3, 1].tolist() == [100, 100, 100]
    _, _, dc = run_emulated(emu, wm, raw, FR.CS16, 1, 256, OUT_HZ, 0, 1, 1, None, [BLK] * 4, 72)
    assert dc[:3, 1].tolist() == [100, 50, 25]           # R = 1: A = 102400, 51200, 25600; (A + 512) >> 10


def check(emu, wm, raw, fmt, R, g, rate, f, cut, tile, tag):
    L, M, taps = design(wm, rate)
    fin = rate or OUT_HZ
    want, clips, dc = DR.convert(raw, fmt, R, fin, f, g, L, M, taps)
    want = want[:want.size // BLK * BLK]
    got, got_clips, got_dc = run_emulated(emu, wm, raw, fmt, R, g, fin, f, L, M, taps, CUTS[cut], tile)
    assert np.array_equal(got_dc, dc), (tag, int(np.argmax(np.any(got_dc != dc, axis=1))))
    assert got.size == want.size, tag
    assert np.array_equal(got, want), (tag, int(np.argmax(got != want)))
    assert got_clips == clips, tag                       # every output counted, the ones behind the last whole block too
    return want, clips, dc


@pytest.mark.parametrize("f", SHIFTS, ids=["noshift", "+250000"])
@pytest.mark.parametrize("R", RS, ids=[f"R{r}" for r in RS])
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fmt, rate, R, f):
    """Every input under the 4096-byte pushes (A carried across every one of them); the offset and the step input, whose dc moves, at
    R = 6 under all three cuts; the random full-range one also at gain x 16."""
    tile = library_tile(emu, wm, fmt, rate)
    clip_seen = 0
    for name, raw in dc_inputs(fmt, N_BLOCKS * BLK).items():
        for cut in list(CUTS) if R == 6 and name in ("offset", "step") else ["each-4096"]:
            want, clips, dc = check(emu, wm, raw, fmt, R, 256, rate, f, cut, tile, (name, cut))
            clip_seen += clips
        if name in ("min", "max"):
            lo, hi = RANGE[fmt][:2]
            x = int(FR.to_x(FR.raw_bytes(np.array([lo if name == "min" else hi] * 2), fmt), fmt)[0, 0])
            assert np.all(dc == x) and np.all(want == 128) and clips == 0      # x' = 0: mid-scale, through every stage
        if name == "offset":
            clip_seen += check(emu, wm, raw, fmt, R, CLIP_GAIN, rate, f, "uneven", tile, (name, "x16"))[1]
    assert clip_seen > 0                                     # the output clamp is reached


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_result_does_not_depend_on_the_tile(emu, wm, fmt, rate):
    """Small odd tiles: many blocks per push, block edges inside level blocks and at every phase of the resampler."""
    raw = dc_inputs(fmt, N_BLOCKS * BLK)["step"]
    tiles = (8, 72, 1000) if rate == 0 else (64, 190)
    for f in SHIFTS:
        for tile in tiles if f == 0 else tiles[1:]:          # the smallest tile is thousands of emulated blocks: once
            check(emu, wm, raw, fmt, 6, CLIP_GAIN, rate, f, "uneven", tile, (f, tile))


def test_without_an_offset_the_blocker_leaves_a_centred_capture_alone(emu, wm):
    """Not through the restatement: a cs16 capture whose every level block sums to zero in I and Q (each block holds a sequence and
    its negative) has dc = 0 throughout, so the bytes are format_ref's bytes of the capture without a blocker."""
    rng = np.random.default_rng(5)
    half = rng.integers(-32767, 32768, (N_BLOCKS * BLK // 4 // DR.BLOCK, DR.BLOCK // 2, 2))
    x = np.concatenate([half, -half], axis=1).reshape(-1, 2)
    raw = FR.raw_bytes(x.reshape(-1), FR.CS16)
    for rate in (0, 2048000):
        L, M, taps = design(wm, rate)
        got, clips, dc = run_emulated(emu, wm, raw, FR.CS16, 6, 300, rate or OUT_HZ, 0, L, M, taps, CUTS["uneven"], library_tile(emu, wm, FR.CS16, rate))
        want, want_clips = FR.convert(raw, FR.CS16, 300, L, M, taps)
        assert np.all(dc == 0) and np.array_equal(got, want[:want.size // BLK * BLK]) and clips == want_clips


YIELD_OFFSET = (12, -9)                              # cu8 steps, smaller than the signal's amplitude of 20


def test_blocker_gives_back_a_capture_that_an_offset_loses(wm, oracle):
    """A medium capture (amplitude 20, noise sigma 3 cu8 steps; 6.4 M samples at 1.6 MS/s) with a constant (+12, -9) added to every
    byte pair: through the restated blocker at R = 6 the oracle must receive at least the clean capture's yield minus 2 % of the
    frames placed (the margin of the resampler's and the gain's yield tests); without the blocker it must stay below that bar.  The
    same capture written as cs8 (s = u - 128: the same x) takes the same road.  Measured: 187 clean, 187 with the blocker, 1 without."""
    kinds = wm.T1 | wm.C1A | wm.C1B | wm.S1
    cu8, frames = wm.synth_capture(seed=77, n_samples=6400000, fs_khz=1600, kinds=kinds, frames_per_s=100.0, amplitude=20.0, noise_sigma=3.0)
    placed = len(frames)
    assert placed >= 150
    opts = oracle.make_opts()
    clean = received(frames, oracle.run(cu8[:cu8.size // BLK * BLK], opts)["text"])
    bad = DR.add_offset_cu8(cu8, *YIELD_OFFSET)
    plain = received(frames, oracle.run(bad[:bad.size // BLK * BLK], opts)["text"])
    y, clips, dc = DR.convert(bad, FR.CU8, 6)
    fixed = received(frames, oracle.run(y[:y.size // BLK * BLK], opts)["text"])
    print(f"of {placed} frames placed: clean {clean}, offset {YIELD_OFFSET} without the blocker {plain}, with input_dc = 6: {fixed}; "
          f"dc I {dc[:, 0].min()} ... {dc[:, 0].max()}, Q {dc[:, 1].min()} ... {dc[:, 1].max()}; clipped {clips}")
    bar = clean - 0.02 * placed
    assert fixed >= bar
    assert plain < bar
    cs8 = FR.raw_bytes(bad.astype(np.int64) - 128, FR.CS8)
    y8, clips8, dc8 = DR.convert(cs8, FR.CS8, 6)
    assert np.array_equal(FR.to_x(cs8, FR.CS8), FR.to_x(bad, FR.CU8))
    fixed8 = received(frames, oracle.run(y8[:y8.size // BLK * BLK], opts)["text"])
    plain8 = received(frames, oracle.run(FR.pipeline_bytes(cs8, FR.CS8), opts)["text"])
    print(f"as cs8: without the blocker {plain8}, with input_dc = 6: {fixed8}")
    assert fixed8 >= bar and plain8 < bar
