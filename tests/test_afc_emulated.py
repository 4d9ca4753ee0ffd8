"""Automatic frequency correction (cfg.input_afc): the ABI; the device source of k0_afc_plan (rtl-wmbus_amd/csrc/wm_k0_afc.h:
k0_afc_plan_block) on the coroutine block emulator against the restatement tests/afc_ref.py, state for state over sequences of pushes; the
AFC form of the two K0-stage kernels (wm_k0_resample.h, AF = true: what k0_resample_afc<> and k0_convert_afc<> run) on the emulator against
the restated bytes, with scripted {step, base}; the equivalence with a fixed shift; and what AFC is for, through the oracle: a capture
tuned off its channel locks in the push that reveals the transmitter and decodes.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import afc_ref as AF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR
from test_formats_emulated import FMT_IDS, FORMATS, design, inputs
from test_resample_emulated import BLK, CUTS, N_BLOCKS
from test_spectrum_emulated import BUNDLED, fields, noise_cu8, surveys  # noqa: F401  (surveys: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libafc_emu.so")
SRC = os.path.join(HERE, "emu", "afc_emu.cpp")
FS = 1600000
OUT_HZ = 1600000
FINS = [800000, 1600000, 2048000, 4000000, 10000000]
IN_RANGE = [-43000, 60000, -30000]                  # the mixes of the bundled capture within the default range
HITS = {-43000: -53674, 60000: 49434, -30000: -43118, 200000: 189719}      # test_survey_then_decode_recovers...: the survey's hit per mix


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_afc: on a library without the field no test of this file says anything, so none passes."""
    assert "input_afc" in [f[0] for f in wm.Cfg._fields_] and "wmbus_read_input_afc" in wm.EXPORTS and hasattr(wm.lib(), "wmbus_read_input_afc")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_the_abi_has_the_afc_fields(wm, tmp_path):
    """The two fields sit directly in front of k1_small_tile, nothing behind them has moved, wmbus_timing keeps its 152 bytes."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_afc")
    assert names[k - 1] == "burst_caps" and names[k + 1:k + 3] == ["input_afc_range_hz", "k1_small_tile"]
    assert names[k + 3:] == ["input_spectrum", "input_channels", "input_channel_hz", "k1_tiles_per_block", "input_agc", "clock_waves", "line_levels",
                             "input_rate_hz", "input_shift_hz", "input_dc", "input_format", "input_gain_q8"]
    types = dict((f[0], f[1]) for f in wm.Cfg._fields_)
    assert types["input_afc"] is ctypes.c_uint and types["input_afc_range_hz"] is ctypes.c_uint
    c = wm.Cfg()
    c.input_afc, c.input_afc_range_hz = 7, 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_afc == 0 and c.input_afc_range_hz == 0
    c = wm._make_cfg(input_afc=1, input_afc_range_hz=50000, input_shift_hz=-7)
    assert (c.input_afc, c.input_afc_range_hz, c.input_shift_hz) == (1, 50000, -7) and wm._make_cfg().input_afc == 0
    assert [f[0] for f in wm.Afc._fields_] == ["shift_hz", "locked", "changes", "ratio_q8"] and ctypes.sizeof(wm.Afc) == 16
    assert hasattr(wm.Receiver, "read_input_afc")
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, input_afc), offsetof(wmbus_cfg, input_afc_range_hz), offsetof(wmbus_cfg, k1_small_tile), sizeof(wmbus_afc), '
                   'sizeof(wmbus_cfg), offsetof(wmbus_afc, ratio_q8));return 0;}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [152, wm.Cfg.input_afc.offset, wm.Cfg.input_afc_range_hz.offset, wm.Cfg.k1_small_tile.offset, 16, ctypes.sizeof(wm.Cfg), 12]
    assert ctypes.sizeof(wm.Timing) == 152 and wm.Cfg.k1_small_tile.offset == wm.Cfg.input_afc.offset + 8
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_afc;", "unsigned input_afc_range_hz;",
                 "typedef struct wmbus_afc { int32_t shift_hz; uint32_t locked, changes, ratio_q8; } wmbus_afc;",
                 "long wmbus_read_input_afc(wmbus_ctx *ctx, unsigned stream, wmbus_afc *out);",
                 "AFC (cfg.input_afc = 1",
                 "cand   = the first hit with |offset_hz - nominal| <= range",
                 "|cand.offset_hz - held_hz| > floor(Fin / 256)",
                 "step   = floor((held_hz 2^32 + Fin / 2) / Fin) mod 2^32",
                 "phase (base + step j) mod 2^32",
                 "base'  = (base + step n_in) mod 2^32",
                 "the result depends on how the input is cut into pushes",
                 "a telegram that straddles a change is rotated with two frequencies",
                 "telegrams in pushes before the first lock are decoded at the nominal",
                 "the max-hold never forgets",
                 "one offset per capture: the strongest transmitter in range wins"):
        assert word in hdr, word
    assert hdr.index("unsigned burst_caps[4];") < hdr.index("unsigned input_afc;") < hdr.index("unsigned input_afc_range_hz;") < hdr.index("unsigned k1_small_tile;")


# ---- k0_afc_plan on the block emulator -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k0_resample.h", "wm_k0_spectrum.h", "wm_k0_afc.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    u, vp, sz = ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t
    L.wm_emu_afc_plan.restype = None
    L.wm_emu_afc_plan.argtypes = [u, ctypes.c_int, u, vp, ctypes.c_uint64, u, vp, vp, u, u]
    L.wm_emu_afc_new.restype = vp
    L.wm_emu_afc_new.argtypes = [u] * 5 + [vp, u, u, vp, u, u, u]
    L.wm_emu_afc_free.argtypes = [vp]
    L.wm_emu_afc_push.restype = ctypes.c_long
    L.wm_emu_afc_push.argtypes = [vp, vp, sz, sz, vp, vp, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_afc_pick_tile.restype = u
    L.wm_emu_afc_pick_tile.argtypes = [u] * 3
    L.wm_emu_afc_convert_tile.restype = u
    L.wm_emu_afc_convert_tile.argtypes = [u]
    L.wm_emu_afc_state_bytes.restype = u
    assert L.wm_emu_afc_state_bytes() == 32
    return L


KEYS = ("held_hz", "locked", "changes", "ratio_q8", "base")


def plan_emulated(emu, fin, nominal, range_hz, st, peak, blocks, n_in, at=1, n_cap=3):
    """k0_afc_plan's block function for the capture at index `at` of `n_cap`: (step, base, the state behind the push)."""
    state = np.array([st[k] % (1 << 32) for k in KEYS], np.uint32)
    push = np.zeros(2, np.uint32)
    pk = np.ascontiguousarray(peak, np.uint32)
    emu.wm_emu_afc_plan(fin, nominal, range_hz or AF.RANGE_HZ, pk.ctypes.data, int(blocks), n_in, state.ctypes.data, push.ctypes.data, at, n_cap)
    out = dict(zip(KEYS, (int(v) for v in state)))
    out["held_hz"] = int(np.int32(state[0]))
    return int(push[0]), int(push[1]), out


def check_sequence(emu, fin, nominal, range_hz, seq, st=None, tag=None):
    """seq: (sum, peak, blocks, n_in) per push.  The emulated kernel against the restatement, state for state; returns the states."""
    ref = emu_st = dict(st) if st else AF.initial(nominal)
    out = []
    for i, (total, peak, blocks, n_in) in enumerate(seq):
        want = AF.plan(fin, nominal, range_hz, ref, total, peak, blocks, n_in)
        got = plan_emulated(emu, fin, nominal, range_hz, emu_st, peak, blocks, n_in, at=i % 3)
        assert got == want, (tag, i, got, want)
        ref, emu_st = want[2], got[2]
        out.append(want)
    return out


def test_plan_on_the_surveys_push_by_push(emu, surveys):
    """Every capture the channel rule is held to, cut into pushes (one level-block-quartet, then more, then the rest): the kernel's
    state against the restatement's after every push, at the capture's own rate and with the default range around the nominal 0; the
    bundled capture's mixes lock where the survey's hit lies, noise never does."""
    for name, (fin, total, peak, blocks, raw) in surveys.items():
        fmt = FR.CS16 if name == "wideband" else FR.CU8
        n = raw.size // BLK
        cuts = [BLK, 7 * BLK, 64 * BLK, (n - 72) * BLK] if n > 80 else [BLK, (n - 1) * BLK]
        states = check_sequence(emu, fin, 0, 0, AF.accumulators(raw, fmt, cuts), tag=name)
        last = states[-1][2]
        print(name, [(s[2]["held_hz"], s[2]["locked"], s[2]["changes"]) for s in states])
        if name.startswith("noise"):
            assert not any(s[2]["locked"] for s in states), name
        for f in IN_RANGE:
            if name == f"samples2{f:+d}":
                assert last["locked"] == 1 and abs(last["held_hz"] - HITS[f]) <= AF.hysteresis(fin)
        if name == "samples2+200000":
            assert last["locked"] == 0 and last["held_hz"] == 0


@pytest.mark.parametrize("fin", FINS)
def test_plan_at_every_rate_and_on_synthetic_max_holds(emu, surveys, fin):
    """The accumulators of the surveys and the synthetic max-holds of test_channels_in_c_equal_the_restated_rule -- flat, edge of the
    band, a tie, all zero, all 0xFFFFFFFF -- as one sequence of pushes at every rate (the rule sees the rate only in W and in
    offset_hz), with a narrow and a wide range, a nominal off zero, a base that wraps, and blocks = 1 and 0."""
    flat = np.full(PR.N, 1000, np.uint32)
    edge = flat.copy(); edge[:20] = 50000; edge[-3:] = 4000000000
    tie = flat.copy(); tie[100:110] = 70000; tie[300:310] = 70000
    low = flat.copy(); low[2:5] = 4000000000                     # a transmitter at the lower edge: offset_hz far below zero
    synth = [np.zeros(PR.N, np.uint32), flat, tie, edge, low, np.full(PR.N, 0xFFFFFFFF, np.uint32)]
    seq = [(pk.astype(np.uint64) * np.uint64(3), pk, 7, 2048 * (i + 1)) for i, pk in enumerate(synth)]
    seq += [(total, peak, blocks, 1 << 22) for _, total, peak, blocks, _ in (surveys[k] for k in ("samples2-43000", "samples2+60000", "wideband", "noise10"))]
    seq += [(seq[2][0], tie, 1, 512), (seq[2][0], tie, 0, 512)]
    half = fin // 2
    n_locked = 0
    for nominal, range_hz in ((0, 0), (0, half), (-(half // 2), half // 2), (fin // 11, 1), (half - 70000, 70000)):
        st = AF.initial(nominal)
        st["base"] = (1 << 32) - 12345
        states = check_sequence(emu, fin, nominal, range_hz, seq, st, tag=(fin, nominal, range_hz))
        n_locked += states[-1][2]["changes"]
        assert states[0][1] == (1 << 32) - 12345                 # the first push starts at the phase the state held, 12345 below the wrap ...
        assert states[1][1] == (states[0][1] + states[0][0] * 2048) % (1 << 32)      # ... and the second where the first ended
    assert n_locked >= 3
    # the tie with the whole band in range: the first hit (the lowest b) is the candidate; with a nominal beside the second, the second
    both = PR.channels(fin, seq[2][0], tie, 7)
    assert len(both) == 2 and both[0]["offset_hz"] < 0 < both[1]["offset_hz"]
    assert check_sequence(emu, fin, 0, half, [seq[2]])[0][2]["held_hz"] == both[0]["offset_hz"]
    near = both[1]["offset_hz"] + 5
    assert check_sequence(emu, fin, near, 100, [seq[2]])[0][2]["held_hz"] == both[1]["offset_hz"]
    # blocks = 0: the rule refuses, nothing locks
    assert check_sequence(emu, fin, 0, half, [(seq[2][0], tie, 0, 512)])[0][2]["locked"] == 0


def test_range_and_hysteresis_to_the_hertz(emu, surveys):
    """A hit exactly at nominal +- range counts, one Hz beyond it does not; a re-estimate exactly floor(Fin / 256) from the held value
    stays, one Hz beyond it moves the lock.  The capture: the bundled one mixed by -43000, hit at -53674 Hz."""
    fin, total, peak, blocks, _ = surveys["samples2-43000"]
    hit = PR.channels(fin, total, peak, blocks)[0]
    h = hit["offset_hz"]
    assert h == HITS[-43000]
    push = (total, peak, blocks, 4096)
    for sign in (1, -1):
        at = check_sequence(emu, fin, h + sign * AF.RANGE_HZ, 0, [push])[0][2]
        beyond = check_sequence(emu, fin, h + sign * (AF.RANGE_HZ + 1), 0, [push])[0][2]
        assert (at["locked"], at["held_hz"], at["ratio_q8"], at["changes"]) == (1, h, hit["ratio_q8"], 1)
        assert (beyond["locked"], beyond["held_hz"], beyond["changes"]) == (0, h + sign * (AF.RANGE_HZ + 1), 0)
        for range_hz in (1000, 1):
            assert check_sequence(emu, fin, h + sign * range_hz, range_hz, [push])[0][2]["locked"] == 1
            assert check_sequence(emu, fin, h + sign * (range_hz + 1), range_hz, [push])[0][2]["locked"] == 0
        hy = AF.hysteresis(fin)
        assert hy == 6250
        held = dict(held_hz=h + sign * hy, locked=1, changes=3, ratio_q8=777, base=0xFFFFF123)
        stays = check_sequence(emu, fin, 0, 0, [push], held)[0]
        assert stays[2] == dict(held, base=(held["base"] + stays[0] * 4096) % (1 << 32)) and stays[0] == SR.step_of(fin, h + sign * hy)
        held["held_hz"] = h + sign * (hy + 1)
        moves = check_sequence(emu, fin, 0, 0, [push], held)[0]
        assert (moves[2]["held_hz"], moves[2]["changes"], moves[2]["ratio_q8"], moves[2]["locked"]) == (h, 4, hit["ratio_q8"], 1)
        assert moves[0] == SR.step_of(fin, h) and moves[1] == 0xFFFFF123       # this push already runs at the new step, from the old phase
        # not locked: the candidate is folded in however near the held value lies
        assert check_sequence(emu, fin, 0, 0, [push], dict(held_hz=h + 1, locked=0, changes=0, ratio_q8=0, base=0))[0][2]["held_hz"] == h


# ---- the AFC form of the stage kernels on the block emulator --------------------------------------------------------------------------

RATES = [0, 2048000]
RATE_IDS = ["native", "2048000"]


def library_tile(emu, wm, fmt, rate):
    if rate == 0:
        return emu.wm_emu_afc_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, OUT_HZ)
    tile = emu.wm_emu_afc_pick_tile(L, M, T)
    assert tile > 0
    return tile


def run_stage(emu, wm, caps, fmt, gain, L, M, taps, cuts, scripts, tile, R=0, agc=0):
    """caps: equally long raw captures; scripts[capture] = (step, base) per push.  Returns (bytes per capture, clip count)."""
    n_cap = len(caps)
    table = wm.shift_design(FS, 0)[1]
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_afc_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile, n_cap, table.ctypes.data, R, agc,
                           max(cuts) // FR.BPS[fmt] // 512)
    assert h
    got, off, clipped = [[] for _ in caps], 0, 0
    try:
        for i, n in enumerate(cuts):
            raw = np.ascontiguousarray(np.stack([c[off:off + n] for c in caps])); off += n
            cap = BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M)
            win = np.full((n_cap, cap + 64), 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            plan = np.array([scripts[k][i] for k in range(n_cap)], np.uint32).reshape(-1)
            r = emu.wm_emu_afc_push(h, raw.ctypes.data, n, n, plan.ctypes.data, win.ctypes.data, cap + 64, cap, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[:, -64:] == 0xA5)
            for k in range(n_cap):
                got[k].append(win[k, :r].copy())
            clipped += clip.value
    finally:
        emu.wm_emu_afc_free(h)
    assert off == caps[0].size
    return [np.concatenate(g) for g in got], clipped


def script_of(fin, fmt, segments, cuts, base0):
    """segments: (raw bytes, held_hz) in stream order -- the state per sample.  cuts: the pushes, each inside one segment.  Returns
    (step, base) per push: the phase runs on from push to push, the step is the segment's."""
    out, base, seg, left = [], base0, 0, segments[0][0]
    for n in cuts:
        if left == 0:
            seg += 1; left = segments[seg][0]
        assert n <= left, "a push straddles a change of state"
        step = SR.step_of(fin, segments[seg][1])
        out.append((step, base))
        base = (base + step * (n // FR.BPS[fmt])) % (1 << 32)
        left -= n
    assert left == 0 and seg == len(segments) - 1
    return out


def whole(y):
    return y[:y.size // BLK * BLK]


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_stage_kernels_follow_a_scripted_lock(emu, wm, fmt, rate):
    """Two captures side by side, each with its own state per sample: unlocked at the nominal -> lock -> change, the phase starting a
    few samples below 2^32 so that the wrap shows.  The sequence cut into pushes in two ways that keep the state per sample (the three
    segments as three pushes; 4096-byte pushes): both give the restated bytes and clip counts -- plain, with input_dc = 6, with
    input_agc."""
    L, M, taps = design(wm, rate)
    fin = rate or OUT_HZ
    tile = library_tile(emu, wm, fmt, rate)
    raw = inputs(fmt, N_BLOCKS * BLK)["random"]
    caps = [raw, np.ascontiguousarray(raw.reshape(-1, FR.BPS[fmt])[::-1].reshape(-1))]
    seg_bytes = CUTS["uneven"]
    helds = [[20000, -53674, -43118], [0, 189719, -200000]]     # per capture: the nominal, a lock, a change
    base0 = [0xFFFFFF00, 0xFFFF0000]
    assert all(abs(a[1] - a[2]) > AF.hysteresis(fin) for a in helds)
    for R, agc, gain in ((0, 0, 300), (6, 0, 256), (0, 1, 0)):
        want, clips = [], 0
        for k, cap in enumerate(caps):
            segs = list(zip(seg_bytes, helds[k]))
            y, c = AF.convert(cap, fmt, seg_bytes, script_of(fin, fmt, segs, seg_bytes, base0[k]), R, agc, gain, L, M, taps)
            want.append(whole(y)); clips += c
        for cut in ("uneven", "each-4096"):
            scripts = [script_of(fin, fmt, list(zip(seg_bytes, helds[k])), CUTS[cut], base0[k]) for k in range(2)]
            assert any(b + s * (n // FR.BPS[fmt]) >= 1 << 32 for (s, b), n in zip(scripts[0], CUTS[cut]))      # the phase wraps inside a push
            got, got_clips = run_stage(emu, wm, caps, fmt, gain, L, M, taps, CUTS[cut], scripts, tile, R, agc)
            for k in range(2):
                assert got[k].size == want[k].size and np.array_equal(got[k], want[k]), (R, agc, cut, k, int(np.argmax(got[k] != want[k])))
            assert got_clips == clips, (R, agc, cut)
        if not R and not agc and fmt in (FR.CS16, FR.CF32):
            assert clips > 0                                     # full-range random input at gain 300 / 256 clips: the count is exercised


@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_constant_lock_is_the_fixed_shift_and_no_lock_the_unshifted_rule(emu, wm, fmt, rate):
    """held_hz constant since the stream's first sample: base = step m, and the bytes and the clip count are those of a context with
    input_shift_hz = held_hz (tests/shift_ref.py), under every cut.  Unlocked at the nominal 0: step 0, entry {16384, 0} -- the bytes
    and the clip count of the unshifted rule (tests/format_ref.py)."""
    L, M, taps = design(wm, rate)
    fin = rate or OUT_HZ
    tile = library_tile(emu, wm, fmt, rate)
    raw = inputs(fmt, N_BLOCKS * BLK)["random"]
    for f, gain in ((-53674, 371), (0, 256)):
        want, clips = (SR.convert(raw, fmt, fin, f, gain, L, M, taps) if f else FR.convert(raw, fmt, gain, L, M, taps))
        for cut in ("one", "uneven", "each-4096"):
            script = script_of(fin, fmt, [(raw.size, f)], CUTS[cut], 0)
            ref = AF.convert(raw, fmt, CUTS[cut], script, 0, 0, gain, L, M, taps)
            assert np.array_equal(ref[0], want) and ref[1] == clips
            got, got_clips = run_stage(emu, wm, [raw], fmt, gain, L, M, taps, CUTS[cut], [script], tile)
            assert np.array_equal(got[0], whole(want)) and got_clips == clips, (f, cut)


# ---- what it is for, through the oracle -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", IN_RANGE, ids=[f"{f:+d}" for f in IN_RANGE])
def test_afc_decodes_a_capture_tuned_off_its_channel(wm, oracle, surveys, f):
    """The bundled capture mixed by f, the whole capture as one push: AFC locks in push 0 at the survey's hit, the bytes are those of
    a fixed shift by that hit, and the oracle on them gives the four lines test_survey_then_decode_recovers... demands -- the first two
    with the golden's identity and payload, at least three CRC-clean.  The capture as it stands gives none."""
    golden = fields(BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"])
    fin, total, peak, blocks, raw = surveys[f"samples2{f:+d}"]
    opts = oracle.make_opts()
    assert oracle.run(raw, opts)["text"] == ""
    hit = PR.channels(fin, total, peak, blocks)[0]
    y, pl = AF.pipeline_bytes(raw, FR.CU8, fin, [raw.size], g_q8=SR.CU8_ROUND_TRIP_GAIN)
    assert len(pl) == 1 and AF.public(pl[0][2]) == dict(shift_hz=hit["offset_hz"], locked=1, changes=1, ratio_q8=hit["ratio_q8"])
    assert hit["offset_hz"] == HITS[f] and pl[0][1] == 0 and pl[0][0] == SR.step_of(fin, HITS[f])
    assert np.array_equal(y, SR.pipeline_bytes(raw, FR.CU8, fin, hit["offset_hz"], SR.CU8_ROUND_TRIP_GAIN))
    got = fields(oracle.run(y, opts)["text"])
    print(f"{f:+d}: lock {pl[0][2]['held_hz']} Hz x{pl[0][2]['ratio_q8'] / 256:.1f}; CRC fields {','.join(g[2] for g in got)}")
    assert len(got) == 4
    assert [g[7:9] for g in got[:2]] == [g[7:9] for g in golden[:2]]
    assert sum(g[2] == "1" for g in got) >= 3


def test_a_transmitter_out_of_range_needs_the_nominal(wm, oracle, surveys):
    """+200000 Hz: with the nominal 0 nothing within +-64 kHz ever locks -- one push or many -- and the bytes are the unshifted rule's;
    with the nominal 200000 the capture locks at the survey's hit, 189719 Hz, and decodes."""
    fin, total, peak, blocks, raw = surveys["samples2+200000"]
    n = raw.size // BLK
    for cuts in ([raw.size], [64 * BLK] * (n // 64) + ([n % 64 * BLK] if n % 64 else [])):
        pl = AF.plans(raw, FR.CU8, fin, cuts)
        assert all(p[2] == AF.initial(0) and p[0] == 0 for p in pl)
    y, pl = AF.pipeline_bytes(raw, FR.CU8, fin, [raw.size], nominal=200000, g_q8=SR.CU8_ROUND_TRIP_GAIN)
    assert AF.public(pl[0][2])["shift_hz"] == HITS[200000] and pl[0][2]["locked"] == 1
    assert len(fields(oracle.run(y, oracle.make_opts())["text"])) == 4


@pytest.mark.parametrize("sigma", [1, 30])
def test_noise_never_locks(sigma):
    """cu8 noise cut into 25 pushes: no push locks, the rotation stays at the nominal."""
    raw = noise_cu8(sigma)
    cuts = [raw.size // 25] * 25
    assert cuts[0] % BLK == 0
    for nominal in (0, -30000):
        pl = AF.plans(raw, FR.CU8, FS, cuts, nominal)
        assert all(p[2]["locked"] == 0 and p[2]["held_hz"] == nominal and p[0] == SR.step_of(FS, nominal) for p in pl)


def test_live_pushes_lock_at_the_first_telegram(wm, oracle, surveys):
    """The bundled capture mixed by -43000 in pushes of 2^18 bytes, what a live stream at 1.6 MS/s delivers: the result depends on the
    cut (the header says so).  The pushes before the first telegram run at the nominal, the push that holds it locks and is decoded
    with the lock, a later and stronger telegram may move it once.
    Measured: 8 pushes; pushes 0 and 1 unlocked, push 2 locks at -53518 Hz x309.6 and nothing moves it afterwards (the whole capture's
    hit, -53674 Hz, lies 0.05 bins away: inside the hysteresis); 4 lines, CRC fields 1,1,1,1 -- the count asserted below as a floor."""
    fin, total, peak, blocks, raw = surveys["samples2-43000"]
    n = raw.size // (1 << 18)
    cuts = [1 << 18] * n + ([raw.size - (n << 18)] if raw.size - (n << 18) else [])
    y, pl = AF.pipeline_bytes(raw, FR.CU8, fin, cuts, g_q8=SR.CU8_ROUND_TRIP_GAIN)
    history, seen = [], 0
    for i, (step, base, st) in enumerate(pl):
        if st["changes"] != seen:
            history.append((i, st["held_hz"], round(st["ratio_q8"] / 256, 1)))
            seen = st["changes"]
    got = fields(oracle.run(y, oracle.make_opts())["text"])
    print(f"{len(cuts)} pushes; lock history {history}; {len(got)} lines, CRC fields {','.join(g[2] for g in got)}")
    assert history and pl[-1][2]["locked"] == 1
    assert abs(pl[-1][2]["held_hz"] - HITS[-43000]) <= 2 * AF.hysteresis(fin)
    assert len(got) >= LIVE_LINES_FLOOR


LIVE_LINES_FLOOR = 4
