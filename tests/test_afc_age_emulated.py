"""The survey that forgets (cfg.input_spectrum_age): the ABI; the AGE form of the survey kernel (rtl-wmbus_amd/csrc/wm_k0_spectrum.h:
k0_spectrum_block<FMT, DC, true>) and the library's own host plan (k0_spec_age_plan) on the coroutine block emulator against the
restatement tests/afc_age_ref.py after every push; k0_afc_plan (wm_k0_afc.h) on the two slots, state for state; and what it is for,
through the oracle: a lock that lets go of a transmitter that has gone silent.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import afc_age_ref as AG
import afc_ref as AF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR
from test_afc_emulated import KEYS
from test_spectrum_emulated import fields

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libafc_age_emu.so")
SRC = os.path.join(HERE, "emu", "afc_age_emu.cpp")
FS = 1600000
BLK = 4096


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_spectrum_age: on a library without the field no test of this file says anything, so none
    passes."""
    assert "input_spectrum_age" in [f[0] for f in wm.Cfg._fields_]


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_the_abi_has_the_age_field(wm, tmp_path):
    """The field sits directly behind bursts_to_host, with input_channel_afc_hz the newest two directly in front of burst_caps; nothing behind them has moved, wmbus_timing keeps its 152
    bytes, the default is 0, the C struct and the ctypes struct agree, and the header defines the view."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_spectrum_age")
    assert names[k - 1] == "bursts_to_host" and names[k + 1:k + 3] == ["input_channel_afc_hz", "burst_caps"]
    assert names[k + 2:] == ["burst_caps", "input_afc", "input_afc_range_hz", "k1_small_tile", "input_spectrum", "input_channels", "input_channel_hz",
                             "k1_tiles_per_block", "input_agc", "clock_waves", "line_levels", "input_rate_hz", "input_shift_hz", "input_dc", "input_format",
                             "input_gain_q8"]
    assert dict((f[0], f[1]) for f in wm.Cfg._fields_)["input_spectrum_age"] is ctypes.c_uint
    c = wm.Cfg()
    c.input_spectrum_age = 9
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_spectrum_age == 0 and wm._make_cfg().input_spectrum_age == 0
    c = wm._make_cfg(input_spectrum=1, input_spectrum_age=12)
    assert (c.input_spectrum, c.input_spectrum_age) == (1, 12)
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, bursts_to_host), offsetof(wmbus_cfg, input_spectrum_age), offsetof(wmbus_cfg, burst_caps), sizeof(wmbus_cfg));return 0;}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [152, wm.Cfg.bursts_to_host.offset, wm.Cfg.input_spectrum_age.offset, wm.Cfg.burst_caps.offset, ctypes.sizeof(wm.Cfg)]
    assert ctypes.sizeof(wm.Timing) == 152 and wm.Cfg.input_spectrum_age.offset == wm.Cfg.bursts_to_host.offset + 4
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_spectrum_age;",
                 "SPECTRUM AGE (cfg.input_spectrum_age = A, 1 ... 31",
                 "e(K) = K >> A",
                 "members  = the level blocks K <= K_last with e(K) in {e_now - 1, e_now} and K >= K_reset",
                 "a reset does not restart it",
                 "wmbus_read_spectrum returns the view",
                 "the max-hold never forgets",
                 "one offset per capture: the strongest transmitter in range wins"):
        assert word in hdr, word
    assert hdr.index("unsigned bursts_to_host;") < hdr.index("unsigned input_spectrum_age;") < hdr.index("unsigned input_channel_afc_hz[WMBUS_MAX_CHANNELS];") < hdr.index("unsigned burst_caps[4];")


# ---- the emulator ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k0_resample.h", "wm_k0_spectrum.h", "wm_k0_afc.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    u, vp, u64 = ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint64
    L.wm_emu_age_host_plan.restype = None
    L.wm_emu_age_host_plan.argtypes = [u64, u, u, ctypes.POINTER(u64), ctypes.POINTER(u)]
    L.wm_emu_age_new.restype = vp
    L.wm_emu_age_new.argtypes = [u, vp, u, u, u, u64]
    L.wm_emu_age_free.argtypes = [vp]
    L.wm_emu_age_push.restype = ctypes.c_long
    L.wm_emu_age_push.argtypes = [vp, vp, ctypes.c_size_t]
    L.wm_emu_age_read.restype = ctypes.c_long
    L.wm_emu_age_read.argtypes = [vp, vp, vp, ctypes.POINTER(u64), ctypes.c_int]
    L.wm_emu_age_slot_blocks.argtypes = [vp, vp]
    L.wm_emu_age_afc_plan.restype = None
    L.wm_emu_age_afc_plan.argtypes = [vp, u, ctypes.c_int, u, u, vp, vp, u, u]
    return L


def host_plan(emu, K_first, n_blk, A):
    e_keep, clear = ctypes.c_uint64(), ctypes.c_uint()
    emu.wm_emu_age_host_plan(K_first, n_blk, A, ctypes.byref(e_keep), ctypes.byref(clear))
    return int(e_keep.value), int(clear.value)


def read_view(emu, h, reset=False):
    total, peak, blocks = np.zeros(PR.N, np.uint64), np.zeros(PR.N, np.uint32), ctypes.c_uint64()
    assert emu.wm_emu_age_read(h, total.ctypes.data, peak.ctypes.data, ctypes.byref(blocks), int(reset)) == PR.N
    return total, peak, int(blocks.value)


def want_view(pw, k_start, K_last, A, K_reset):
    """The view of a stream whose first level block is the context's k_start (pw[0] is level block k_start)."""
    m = AG.members(K_last, A, max(K_reset, k_start))
    part = pw[m.start - k_start:m.stop - k_start] if len(m) else pw[:0]
    return part.sum(axis=0).astype(np.uint64), part.max(axis=0, initial=0).astype(np.uint32), len(m)


def same(a, b):
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def run_pushes(emu, wm, raw, pw, fmt, R, A, run, cuts_blocks, k_start=0, resets=()):
    """The emulated kernel over the pushes (level blocks each), the view after every push held against the restatement.  Returns
    {K_last: view}."""
    per = PR.N * FR.BPS[fmt]
    table = wm.shift_design(FS, 0)[1]
    h = emu.wm_emu_age_new(fmt, table.ctypes.data, R, run, A, k_start)
    out, off, K_reset = {}, 0, k_start
    try:
        for i, n in enumerate(cuts_blocks):
            part = np.ascontiguousarray(raw[off * per:(off + n) * per]); off += n
            assert emu.wm_emu_age_push(h, part.ctypes.data, part.size) == n
            K_last = k_start + off - 1
            got = read_view(emu, h, reset=i in resets)
            want = want_view(pw, k_start, K_last, A, K_reset)
            assert got[2] == want[2], (A, run, i, got[2], want[2])
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (A, run, i)
            out[K_last] = got
            if i in resets:
                K_reset = K_last + 1
    finally:
        emu.wm_emu_age_free(h)
    return out


def shapes(cuts_blocks, k_start, A, run):
    """Which of the push shapes the kernel and the host plan must get right occur in a sequence of pushes."""
    seen, K = set(), k_start
    for i, n in enumerate(cuts_blocks):
        first_e, last_e = K >> A, (K + n - 1) >> A
        if i == 0 and n < (1 << A):
            seen.add("first push shorter than an epoch")
        if first_e == last_e and (K + n) % (1 << A):
            seen.add("inside one epoch")
        if (K + n) % (1 << A) == 0:
            seen.add("ends on an edge")
        if last_e == first_e + 1:
            seen.add("crosses one edge")
        if last_e >= first_e + 3:
            seen.add("spans four epochs")
        if any((e << A) > K and ((e << A) - K) % run for e in range(first_e + 1, last_e + 1)):
            seen.add("an edge inside a wave's run")
        K += n
    return seen


ALL_SHAPES = {"first push shorter than an epoch", "inside one epoch", "ends on an edge", "crosses one edge", "spans four epochs", "an edge inside a wave's run"}
N_STREAM = 72                                       # level blocks of the test stream
CUTS_A = [2, 6, 4, 8, 40, 2, 6, 4]                  # level blocks per push: with A = 3 every shape above (asserted below)
CUTS_B = [8, 4, 12, 36, 8, 4]                       # another cut of the same stream with K_last in common
STREAM_FORMATS = [(FR.CU8, 0), (FR.CS16, 0), (FR.CS16, 6)]
_STREAMS = {}


def stream(fmt, R):
    """(raw, pw) of the test stream, the restated power computed once per format."""
    if (fmt, R) not in _STREAMS:
        rng = np.random.default_rng(0xA6E + fmt)
        n = N_STREAM * PR.N
        t = np.arange(n)
        z = 0.02 * (rng.normal(size=n) + 1j * rng.normal(size=n)) + 0.4 * np.exp(2j * np.pi * (t // (7 * PR.N) % 5 - 2) * 0.07 * t)    # a tone that hops
        v = np.stack([z.real + 0.1, z.imag - 0.05], axis=1).reshape(-1)
        raw = (np.clip(np.rint(127.5 + 127.0 * v), 0, 255).astype(np.uint8) if fmt == FR.CU8
               else FR.raw_bytes(np.clip(np.rint(30000.0 * v), -32768, 32767).astype(np.int16), fmt))
        _STREAMS[(fmt, R)] = (raw, AG.stream_power(raw, fmt, R))
    return _STREAMS[(fmt, R)]


def test_the_cuts_hold_every_push_shape():
    assert sum(CUTS_A) == sum(CUTS_B) == N_STREAM
    for run in (3, 4, 16):
        assert shapes(CUTS_A, 0, 3, run) == ALL_SHAPES, (run, ALL_SHAPES - shapes(CUTS_A, 0, 3, run))
    assert "an edge inside a wave's run" in shapes(CUTS_A, 5, 3, 4)
    # pushes of whole 4096-byte blocks: 4 level blocks of cu8, 2 of cs16
    assert all(n % 2 == 0 for n in CUTS_A + CUTS_B) and all(n % 4 == 0 for n in CUTS_B)


@pytest.mark.parametrize("run", [1, 3, 4, 16])
@pytest.mark.parametrize("A", [1, 2, 3, 5])
@pytest.mark.parametrize("fmt,R", STREAM_FORMATS, ids=["cu8", "cs16", "cs16-dc6"])
def test_aged_kernel_gives_the_view_after_every_push(emu, wm, fmt, R, A, run):
    """The AGE form and the library's host plan against view() after every push: pushes inside one epoch, ending on an edge, crossing
    one, spanning four or more (level blocks are left out and both slots cleared), edges inside a wave's run, a first push shorter than
    an epoch; a second cut of the same stream gives the same view wherever the two have a K_last in common; and the same stream as
    the continuation of a long one (K_first = 2^40 + 5: the 64 bits of K, and a K_first that is no multiple of the run)."""
    raw, pw = stream(fmt, R)
    cuts_a = CUTS_A if fmt != FR.CU8 else [2 * n for n in CUTS_B[:3]] + [N_STREAM - 2 * sum(CUTS_B[:3])]
    a = run_pushes(emu, wm, raw, pw, fmt, R, A, run, cuts_a)
    b = run_pushes(emu, wm, raw, pw, fmt, R, A, run, CUTS_B)
    common = set(a) & set(b)
    assert len(common) >= 2 and all(same(a[k], b[k]) for k in common)
    if R == 0:                                                   # (the blocker's recurrence starts with the stream: it has no k_start)
        k0 = (1 << 40) + 5
        c = run_pushes(emu, wm, raw, pw, fmt, R, A, run, cuts_a, k_start=k0)
        assert all(c[k][2] >= min((1 << A) + 1, k - k0 + 1) for k in c)       # between E + 1 and 2 E level blocks once the stream is that long
        assert all(c[k][2] <= 2 << A for k in c)


@pytest.mark.parametrize("A", [2, 3])
def test_a_reset_in_mid_stream(emu, wm, A):
    """wmbus_read_spectrum(reset) behind pushes 1 and 4: the view holds only level blocks behind the last reset, K runs on."""
    raw, pw = stream(FR.CS16, 0)
    for run in (3, 4):
        run_pushes(emu, wm, raw, pw, FR.CS16, 0, A, run, CUTS_A, resets=(1, 4))
    assert want_view(pw, 0, 11, A, 8)[2] == 4                    # push 2 behind the reset at K = 8: its own 4 level blocks alone


def test_age_31_is_the_survey_that_never_forgets(emu, wm):
    """A = 31 over a short stream: one epoch, nothing is ever cleared or left out -- today's arrays (tests/spectrum_ref.py)."""
    raw, pw = stream(FR.CU8, 0)
    got = run_pushes(emu, wm, raw, pw, FR.CU8, 0, 31, 4, [4 * n for n in (1, 3, 2, 12)])
    assert same(got[N_STREAM - 1], PR.spectrum(raw, FR.CU8))
    assert same(AG.view(pw, N_STREAM - 1, 0), PR.spectrum(raw, FR.CU8))


def test_the_host_plan_on_its_own(emu):
    """k0_spec_age_plan, the function wm_api.hip calls, on slots held as sets of level-block indices: after every push the slots
    together are the members of the view, each slot holds one epoch, and nothing is cleared that the view still needs -- over the test's
    cuts, random cuts, pushes of one level block and of many epochs, every A of the kernel test and 31, K from 0 and from 2^40 + 5."""
    rng = np.random.default_rng(31)
    sequences = [CUTS_A, CUTS_B, [1] * 40, [100, 1, 1, 300, 7]] + [list(rng.integers(1, 70, 30)) for _ in range(20)]
    n_clear = {0: 0, 1: 0, 2: 0, 3: 0}
    for A in (1, 2, 3, 5, 31):
        for k_start in (0, 5, (1 << 40) + 5):
            for cuts in sequences:
                slots, K = [set(), set()], k_start
                for n in cuts:
                    n = int(n)
                    e_keep, clear = host_plan(emu, K, n, A)
                    assert e_keep == max(((K + n - 1) >> A) - 1, 0) and clear in (0, 1, 2, 3)
                    n_clear[clear] += 1
                    AG.apply_plan(slots, K, n, A, e_keep, clear)
                    K += n
                    assert slots[0] | slots[1] == set(AG.members(K - 1, A, k_start)), (A, k_start, K, n)
                    for s in range(2):
                        assert len({k >> A for k in slots[s]}) <= 1 and all((k >> A) & 1 == s for k in slots[s])
    assert all(n_clear.values())                                 # nothing, either slot alone and both: every answer occurs


# ---- the plan on the view ----------------------------------------------------------------------------------------------------------

def history(pl):
    """[(push, held_hz)] of the pushes that changed the lock."""
    out, seen = [], 0
    for i, (_, _, st) in enumerate(pl):
        if st["changes"] != seen:
            out.append((i, st["held_hz"]))
            seen = st["changes"]
    return out


HALF_BIN = FS / PR.N / 2                             # the rule's centroid lies within half a survey bin of a lone tone


def test_the_lock_lets_go_of_a_transmitter_that_is_gone(emu, wm):
    """cu8 at 1.6 MS/s, six pushes of 8 x 4096 bytes (32 level blocks), noise sigma 0.004; a tone of amplitude 0.5 at +25 kHz in pushes
    0-1, a tone of amplitude 0.1 at -20 kHz from push 2 on.  From the restatement alone: the survey that never forgets holds the first
    lock through all six pushes; A = 5 (the view: this push and the one before it) moves at push 3, A = 3 (a push spans four epochs: the
    view is its last 16 level blocks) at push 2, A = 6 at push 4.  Then the emulated kernels -- the AGE survey, the plan on the two slots
    -- state for state against the restatement."""
    raw, cuts = AG.two_tones()
    n_in = cuts[0] // 2
    hist = {A: history(AG.plans(raw, FR.CU8, FS, cuts, A)) for A in (0, 3, 5, 6)}
    print(hist)
    first = hist[0][0][1]
    assert hist[0] == [(0, first)] and abs(first - 25000) < HALF_BIN and AG.plans(raw, FR.CU8, FS, cuts, 0) == AF.plans(raw, FR.CU8, FS, cuts)
    for A, moves_at in ((5, 3), (3, 2), (6, 4)):
        assert [h[0] for h in hist[A]] == [0, moves_at] and hist[A][0][1] == first and abs(hist[A][1][1] + 20000) < HALF_BIN, (A, hist[A])
    assert [len(AG.members(32 * (i + 1) - 1, 3)) for i in range(6)] == [16] * 6
    table = wm.shift_design(FS, 0)[1]
    for A in (3, 5, 6):
        want = AG.plans(raw, FR.CU8, FS, cuts, A)
        h = emu.wm_emu_age_new(FR.CU8, table.ctypes.data, 0, 4, A, 0)
        try:
            st = AF.initial(0)
            for i, n in enumerate(cuts):
                part = np.ascontiguousarray(raw[i * n:(i + 1) * n])
                assert emu.wm_emu_age_push(h, part.ctypes.data, part.size) == 32
                state = np.array([st[k] % (1 << 32) for k in KEYS], np.uint32)
                push = np.zeros(2, np.uint32)
                emu.wm_emu_age_afc_plan(h, FS, 0, AF.RANGE_HZ, n_in, state.ctypes.data, push.ctypes.data, i % 3, 3)
                st = dict(zip(KEYS, (int(v) for v in state)))
                st["held_hz"] = int(np.int32(state[0]))
                assert (int(push[0]), int(push[1]), st) == want[i], (A, i)
        finally:
            emu.wm_emu_age_free(h)


# ---- what it is for, through the oracle ----------------------------------------------------------------------------------------------

SECOND_HALF_AMPLITUDE = 0.5                          # of the bundled capture's own
AGED_LINES_FLOOR = 8                                 # measured, see the test


def test_a_drifted_receiver_is_followed_where_the_survey_forgets(wm, oracle, samples):
    """The bundled capture mixed by -43000 Hz, followed by the same capture mixed by +40000 Hz at half the amplitude, in pushes of 2^18
    bytes: a receiver that has moved by 83 kHz and hears its transmitter weaker than before.  The second half alone, with its own fixed
    shift, decodes (checked first).  With the survey that never forgets the lock stays on the first half's hit and the second half
    yields no line; with A = 8 (epochs of 256 level blocks, one push: the view is the last two pushes) the lock moves and the second half
    is decoded.
    Measured: 16 pushes of 256 level blocks.  A = 0: lock history [(2, -53518)], 4 + 0 lines (first half + second half).  A = 8: lock
    history [(2, -53518), (10, 28725)] -- push 10 holds the second half's first telegram, and the view, pushes 9 and 10, is free of the
    first half by then -- 4 + 4 lines: the total asserted below as a floor."""
    s2 = samples["samples2"]
    s2 = s2[:s2.size // (1 << 18) * (1 << 18)]
    first = SR.round_trip_cu8(s2, FS, -43000)
    x = SR.round_trip_cu8(s2, FS, 40000).astype(np.float64) - 127.5
    second = np.clip(np.rint(127.5 + SECOND_HALF_AMPLITUDE * x), 0, 255).astype(np.uint8)
    opts = oracle.make_opts()
    hit = PR.channels(FS, *PR.spectrum(second, FR.CU8))[0]["offset_hz"]
    alone = fields(oracle.run(SR.pipeline_bytes(second, FR.CU8, FS, hit, SR.CU8_ROUND_TRIP_GAIN), opts)["text"])
    assert len(alone) >= 3, "the second half must be decodable with its own shift"
    raw = np.concatenate([first, second])
    cuts = [1 << 18] * (raw.size >> 18)
    result = {}
    for A in (0, 8):
        assert A == 0 or 2 * (512 << A) < first.size             # two epochs are shorter than half the stream
        y, pl = AG.pipeline_bytes(raw, FR.CU8, FS, cuts, A, g_q8=SR.CU8_ROUND_TRIP_GAIN)
        y1, y2 = y[:first.size], y[first.size:]
        lines1, lines2 = fields(oracle.run(y1, opts)["text"]), fields(oracle.run(y2, opts)["text"])
        result[A] = (history(pl), len(lines1), len(lines2))
        print(f"A = {A}: {len(cuts)} pushes; lock history {result[A][0]}; {len(lines1)} + {len(lines2)} lines")
    assert len(result[0][0]) == 1 and result[0][2] == 0          # the lock never moves: the second half is lost
    assert len(result[8][0]) == 2 and abs(result[8][0][1][1] - hit) <= 2 * AF.hysteresis(FS)
    assert result[8][2] >= 1 and result[8][1] + result[8][2] > result[0][1] + result[0][2]
    assert result[8][1] + result[8][2] >= AGED_LINES_FLOOR


# ---- a lock per channel (cfg.input_channel_afc_hz) ---------------------------------------------------------------------------------------

import channels_fixture as CF                                              # noqa: E402
from test_afc_emulated import script_of, whole                             # noqa: E402
from test_formats_emulated import FMT_IDS, FORMATS, design, inputs         # noqa: E402
from test_resample_emulated import CUTS, N_BLOCKS                          # noqa: E402

CH_HZ = [700000, -600000, 0]
CH_RANGE = [64000, 0, 20000]


@pytest.fixture()
def the_library_has_the_channel_field(wm):
    assert "input_channel_afc_hz" in [f[0] for f in wm.Cfg._fields_]


def test_the_abi_has_the_channel_afc_field(wm, tmp_path, the_library_has_the_channel_field):
    """The array sits behind input_spectrum_age and directly in front of burst_caps; the default is all 0; _make_cfg takes a list; the C
    struct and the ctypes struct agree; the header holds the contract."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_channel_afc_hz")
    assert names[k - 2:k + 2] == ["bursts_to_host", "input_spectrum_age", "input_channel_afc_hz", "burst_caps"]
    c = wm.Cfg()
    for i in range(wm.MAX_CHANNELS):
        c.input_channel_afc_hz[i] = 7
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert list(c.input_channel_afc_hz) == [0] * wm.MAX_CHANNELS and list(wm._make_cfg().input_channel_afc_hz) == [0] * wm.MAX_CHANNELS
    c = wm._make_cfg(input_channel_hz=CH_HZ, input_channel_afc_hz=CH_RANGE)
    assert list(c.input_channel_afc_hz)[:4] == CH_RANGE + [0] and c.input_channels == 3 and c.input_afc == 0
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, input_spectrum_age), offsetof(wmbus_cfg, input_channel_afc_hz), offsetof(wmbus_cfg, burst_caps), sizeof(wmbus_cfg));return 0;}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [152, wm.Cfg.input_spectrum_age.offset, wm.Cfg.input_channel_afc_hz.offset, wm.Cfg.burst_caps.offset, ctypes.sizeof(wm.Cfg)]
    assert wm.Cfg.burst_caps.offset == wm.Cfg.input_channel_afc_hz.offset + 4 * wm.MAX_CHANNELS
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_channel_afc_hz[WMBUS_MAX_CHANNELS];",
                 "CHANNEL AFC (cfg.input_channel_afc_hz[c] = range of channel c, 0: the channel is fixed",
                 "pipeline stream v = k C + c (capture k, channel c) carries an AFC state of its own",
                 "a channel with range 0 skips the search",
                 "Two channels may lock on the same transmitter",
                 "more than rel (8) times weaker than the capture's strongest hit is not reported",
                 "one offset per capture: the strongest transmitter in range wins"):
        assert word in hdr, word


def bind_channel_emu(L):
    u, vp, sz = ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t
    L.wm_emu_chafc_plan.restype = None
    L.wm_emu_chafc_plan.argtypes = [u, u, u, vp, vp, vp, vp, u, vp, vp]
    L.wm_emu_chafc_new.restype = vp
    L.wm_emu_chafc_new.argtypes = [u] * 5 + [vp, u, u, u, vp, u, u, u]
    L.wm_emu_chafc_free.argtypes = [vp]
    L.wm_emu_chafc_push.restype = ctypes.c_long
    L.wm_emu_chafc_push.argtypes = [vp, vp, sz, sz, vp, vp, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_chafc_pick_tile.restype = u
    L.wm_emu_chafc_pick_tile.argtypes = [u] * 3
    L.wm_emu_chafc_convert_tile.restype = u
    L.wm_emu_chafc_convert_tile.argtypes = [u]
    return L


def channel_plan_emulated(emu, fin, hz, ranges, states, peaks, blocks, n_in):
    """k0_afc_plan on the grid (captures, channels): states[v] in, (step, base, state) per v out."""
    bind_channel_emu(emu)
    n_cap, n_ch = len(peaks), len(hz)
    st = np.array([[s[k] % (1 << 32) for k in KEYS] for s in states], np.uint32)
    push = np.zeros((n_cap * n_ch, 2), np.uint32)
    pk = np.ascontiguousarray(np.stack(peaks), np.uint32)
    bl = np.array(blocks, np.uint64)
    nominal, rng = np.array(hz, np.int32), np.array(ranges, np.uint32)
    emu.wm_emu_chafc_plan(fin, n_cap, n_ch, nominal.ctypes.data, rng.ctypes.data, pk.ctypes.data, bl.ctypes.data, n_in, st.ctypes.data, push.ctypes.data)
    out = []
    for v in range(n_cap * n_ch):
        d = dict(zip(KEYS, (int(x) for x in st[v])))
        d["held_hz"] = int(np.int32(st[v, 0]))
        out.append((int(push[v, 0]), int(push[v, 1]), d))
    return out


def tones_cs16(fin, n, parts, seed):
    """cs16 raw bytes: noise of sigma 0.004 and tones (Hz, amplitude, first sample, last sample)."""
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    z = 0.004 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    for f, a, first, last in parts:
        z = z + a * np.exp(2j * np.pi * (f / fin) * t) * ((t >= first) & (t < last))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    return FR.raw_bytes(np.clip(np.rint(30000.0 * v), -32768, 32767).astype(np.int16), FR.CS16)


def two_wide_captures(fin=CF.WIDE_FS, push=8 * BLK, pushes=3):
    """Two cs16 captures at 4.0 MS/s for the list CH_HZ / CH_RANGE, three pushes of 16 level blocks.  Capture 0: transmitters 15 kHz above
    channel 0 (in range: locks in push 0), 5 kHz above channel 1 (fixed: ignored), 30 kHz above channel 2 (beyond its 20 kHz: never
    locks).  Capture 1: 50 kHz below channel 0 from push 1 on, and 10 kHz below channel 2; in push 2 a twice as strong one 12 kHz above
    channel 2: its lock moves."""
    n = push // 4
    a = tones_cs16(fin, pushes * n, [(715000, 0.2, 0, 3 * n), (-595000, 0.2, 0, 3 * n), (30000, 0.2, 0, 3 * n)], 61)
    b = tones_cs16(fin, pushes * n, [(650000, 0.2, n, 3 * n), (-10000, 0.15, 0, 3 * n), (12000, 0.3, 2 * n, 3 * n)], 62)
    return [a, b], [push] * pushes


def test_channel_plan_state_for_state(emu, the_library_has_the_channel_field):
    """C = 3 with ranges [64000, 0, 20000] over two captures and three pushes: the emulated plan kernel on its grid (captures, channels)
    against the restatement, state per pipeline stream v.  The fixed channel never locks and its base is step x m."""
    fin = CF.WIDE_FS
    caps, cuts = two_wide_captures()
    want = [AG.channel_plans(c, FR.CS16, fin, cuts, CH_HZ, CH_RANGE) for c in caps]          # [capture][channel][push]
    acc = [AF.accumulators(c, FR.CS16, cuts) for c in caps]
    # from the restatement alone: what the test is about does occur
    last = [[want[k][c][-1][2] for c in range(3)] for k in range(2)]
    assert last[0][0]["locked"] == 1 and abs(last[0][0]["held_hz"] - 715000) < fin / PR.N / 2 and want[0][0][0][2]["locked"] == 1
    assert last[0][2]["locked"] == 0 and last[0][2]["held_hz"] == 0
    assert [p[2]["locked"] for p in want[1][0]] == [0, 1, 1] and abs(last[1][0]["held_hz"] - 650000) < fin / PR.N / 2
    assert [p[2]["changes"] for p in want[1][2]] == [1, 1, 2]
    states = [AF.initial(CH_HZ[v % 3]) for v in range(6)]
    m = 0
    for i, n in enumerate(cuts):
        n_in = n // 4
        got = channel_plan_emulated(emu, fin, CH_HZ, CH_RANGE, states, [acc[k][i][1] for k in range(2)], [acc[k][i][2] for k in range(2)], n_in)
        for v in range(6):
            assert got[v] == want[v // 3][v % 3][i], (i, v, got[v], want[v // 3][v % 3][i])
        for k in range(2):                                       # the fixed channel: {hz, 0, 0, 0}, the phase of a fixed shift
            step, base, st = got[3 * k + 1]
            assert AF.public(st) == dict(shift_hz=CH_HZ[1], locked=0, changes=0, ratio_q8=0)
            assert step == SR.step_of(fin, CH_HZ[1]) and base == step * m % (1 << 32)
        states = [g[2] for g in got]
        m += n_in


@pytest.mark.parametrize("fin", [1600000, 4000000])
def test_channel_plan_on_synthetic_max_holds(emu, fin, the_library_has_the_channel_field):
    """The synthetic max-holds of the per-capture plan's test -- all zero, flat, a tie, an edge of the band, the lower edge, all
    0xFFFFFFFF -- as pushes of two captures (the second sees them in reverse order), with two channels whose ranges overlap and a
    third that is fixed: state per v against the restatement; on the tie both following channels lock on the same transmitter."""
    flat = np.full(PR.N, 1000, np.uint32)
    edge = flat.copy(); edge[:20] = 50000; edge[-3:] = 4000000000
    tie = flat.copy(); tie[100:110] = 70000; tie[300:310] = 70000
    low = flat.copy(); low[2:5] = 4000000000
    synth = [np.zeros(PR.N, np.uint32), flat, tie, edge, low, np.full(PR.N, 0xFFFFFFFF, np.uint32)]
    half = fin // 2
    hz, ranges = [-(fin // 16), fin // 16, fin // 5], [half - fin // 16, half - fin // 16, 0]
    states = [dict(AF.initial(hz[v % 3]), base=(1 << 32) - 999 * (v + 1)) for v in range(6)]
    ref = [dict(s) for s in states]
    same_lock = 0
    for i in range(len(synth)):
        peaks = [synth[i], synth[len(synth) - 1 - i]]
        blocks = [7, 0 if i == 3 else 5]                         # blocks = 0: the rule refuses, nothing locks in that push
        n_in = 2048 * (i + 1)
        got = channel_plan_emulated(emu, fin, hz, ranges, states, peaks, blocks, n_in)
        for v in range(6):
            k, c = divmod(v, 3)
            want = AG.channel_plan(fin, hz[c], ranges[c], ref[v], peaks[k].astype(np.uint64) * np.uint64(3), peaks[k], blocks[k], n_in)
            assert got[v] == want, (fin, i, v, got[v], want)
            ref[v] = want[2]
        states = [g[2] for g in got]
        if peaks[0] is tie:
            both = PR.channels(fin, tie.astype(np.uint64), tie, 7)
            assert len(both) == 2 and states[0]["held_hz"] == states[1]["held_hz"] == both[0]["offset_hz"] and states[0]["locked"] == states[1]["locked"] == 1
            same_lock += 1
    assert same_lock == 1 and all(states[v]["locked"] == 0 and states[v]["held_hz"] == hz[2] for v in (2, 5))


def run_channel_stage(emu, wm, caps, n_ch, fmt, gain, L, M, taps, cuts, scripts, tile, R=0, agc=0):
    """caps: equally long raw captures; scripts[v] = (step, base) per push for v = capture x n_ch + channel.  Returns (bytes per v, clip
    count over all v)."""
    bind_channel_emu(emu)
    n_cap, nv = len(caps), len(caps) * n_ch
    table = wm.shift_design(FS, 0)[1]
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    h = emu.wm_emu_chafc_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile, n_cap, n_ch, table.ctypes.data, R, agc,
                             max(cuts) // FR.BPS[fmt] // 512)
    assert h
    got, off, clipped = [[] for _ in range(nv)], 0, 0
    try:
        for i, n in enumerate(cuts):
            raw = np.ascontiguousarray(np.stack([c[off:off + n] for c in caps])); off += n
            cap = BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M)
            win = np.full((nv, cap + 64), 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            plan = np.array([scripts[v][i] for v in range(nv)], np.uint32).reshape(-1)
            r = emu.wm_emu_chafc_push(h, raw.ctypes.data, n, n, plan.ctypes.data, win.ctypes.data, cap + 64, cap, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[:, -64:] == 0xA5)
            for v in range(nv):
                got[v].append(win[v, :r].copy())
            clipped += clip.value
    finally:
        emu.wm_emu_chafc_free(h)
    assert off == caps[0].size
    return [np.concatenate(g) for g in got], clipped


@pytest.mark.parametrize("rate", [0, 2048000], ids=["native", "2048000"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_channel_stage_kernels_follow_a_script_per_stream(emu, wm, fmt, rate, the_library_has_the_channel_field):
    """The CH && AF form of the two stage kernels, two captures x three channels: channels 0 and 2 with a scripted state per sample
    (nominal -> lock -> change, the phase wrapping inside a push), channel 1 fixed ({step of its Hz, step x m}); plain, with
    input_dc = 6, with input_agc; the sequence cut in two ways.  Bytes and clip count of every pipeline stream equal tests/afc_ref.py's
    with that stream's script; the fixed channel equals the channels restatement (tests/channels_fixture.py)."""
    L, M, taps = design(wm, rate)
    fin = rate or FS
    bind_channel_emu(emu)
    tile = emu.wm_emu_chafc_convert_tile(fmt) if rate == 0 else emu.wm_emu_chafc_pick_tile(*wm.resampler_design(rate, FS)[:3])
    assert tile > 0
    raw = inputs(fmt, N_BLOCKS * BLK)["random"]
    caps = [raw, np.ascontiguousarray(raw.reshape(-1, FR.BPS[fmt])[::-1].reshape(-1))]
    seg_bytes = CUTS["uneven"]
    fixed_hz = -250000
    helds = [[20000, -53674, -43118], None, [0, 189719, -200000], [-30000, 40000, 60000], None, [100000, 100000, 93000]]     # per v
    base0 = [0xFFFFFF00, 0, 0xFFFF0000, 0xFFFFF000, 0, 12345]

    def script(v, cuts):
        segs = [(raw.size, fixed_hz)] if helds[v] is None else list(zip(seg_bytes, helds[v]))
        return script_of(fin, fmt, segs, cuts, base0[v])

    for R, agc, gain in ((0, 0, 300), (6, 0, 256), (0, 1, 0)):
        want, clips = [], 0
        for v in range(6):
            y, c = AF.convert(caps[v // 3], fmt, seg_bytes, script(v, seg_bytes), R, agc, gain, L, M, taps)
            want.append(whole(y)); clips += c
        for k in range(2):                                       # the fixed channel: what a channels context gives for it
            y, c = CF.restated(caps[k], fmt, fin, fixed_hz, gain or 256, L, M, taps, R, agc)[:2]
            assert np.array_equal(whole(y), want[3 * k + 1])
        for cut in ("uneven", "each-4096"):
            scripts = [script(v, CUTS[cut]) for v in range(6)]
            assert any(b + s * (n // FR.BPS[fmt]) >= 1 << 32 for (s, b), n in zip(scripts[0], CUTS[cut]))      # the phase wraps inside a push
            got, got_clips = run_channel_stage(emu, wm, caps, 3, fmt, gain, L, M, taps, CUTS[cut], scripts, tile, R, agc)
            for v in range(6):
                assert got[v].size == want[v].size and np.array_equal(got[v], want[v]), (R, agc, cut, v, int(np.argmax(got[v] != want[v])))
            assert got_clips == clips, (R, agc, cut)


WIDE_OFF_HZ = [730000, -625000, 0]                   # where the three transmitters really sit
CHANNEL_LINES_FLOOR = [8, 9, 6]                      # measured, see the test


def test_channel_afc_decodes_a_wideband_capture_tuned_off_its_list(wm, oracle, the_library_has_the_channel_field):
    """The three-channel wideband capture with its transmitters at 730000, -625000 and 0 Hz, decoded with the list [700000, -600000, 0]
    and ranges of 64000, the whole capture as one push: every channel locks at its survey hit, every channel's bytes are those of a
    fixed shift at its lock, and the oracle on them gives more lines in total than on the bytes of the fixed list.
    Measured: locks 728431, -628922 and 191 Hz; lines per channel 8, 9, 6 with the locks -- the counts asserted below as floors --
    against 4, 8, 6 with the fixed list (the reference still decodes most of a channel 25 kHz off, half of one 30 kHz off)."""
    raw = CF.wideband(wm, hz=WIDE_OFF_HZ)[0]
    fin = CF.WIDE_FS
    L, M, T, taps = wm.resampler_design(fin, FS)
    pl = AG.channel_plans(raw, FR.CS16, fin, [raw.size], CF.WIDE_HZ, [64000] * 3)
    opts = oracle.make_opts()
    n_afc, n_fixed, locks = [], [], []
    for c in range(3):
        step, base, st = pl[c][0]
        assert st["locked"] == 1 and base == 0 and abs(st["held_hz"] - WIDE_OFF_HZ[c]) < fin / PR.N
        locks.append(st["held_hz"])
        y, _ = AF.convert(raw, FR.CS16, [raw.size], [(step, base)], 0, 0, CF.WIDE_GAIN, L, M, taps)
        at_lock = CF.restated(raw, FR.CS16, fin, st["held_hz"], CF.WIDE_GAIN, L, M, taps)[0]
        assert np.array_equal(y, at_lock)
        n_afc.append(len(fields(oracle.run(whole(y), opts)["text"])))
        n_fixed.append(len(fields(oracle.run(whole(CF.restated(raw, FR.CS16, fin, CF.WIDE_HZ[c], CF.WIDE_GAIN, L, M, taps)[0]), opts)["text"])))
    print(f"locks {locks}; lines per channel with the locks {n_afc}, with the fixed list {n_fixed}")
    assert all(a >= f for a, f in zip(n_afc, CHANNEL_LINES_FLOOR))
    assert sum(n_afc) > sum(n_fixed)
