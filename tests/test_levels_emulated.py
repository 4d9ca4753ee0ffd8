"""Line levels (cfg.line_levels): the ABI; the device source of k3_levels and k3_level_tail (rtl-wmbus_amd/csrc/wm_k3_levels.h) on the
coroutine block emulator against the numpy restatement tests/level_ref.py, record for record; and what the measurement is for, on the
oracle alone: the median offset over a capture's telegrams tracks the offset the generator gave them.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import level_ref as LR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "liblevel_emu.so")
SRC = os.path.join(HERE, "emu", "level_emu.cpp")

LEVEL_DTYPE = np.dtype([("sync_sample", "<u8"), ("offset_hz", "<i4"), ("dev_hz", "<u4"), ("n", "<u4"), ("pad", "<u4")])
PKT_RLA, PKT_T2A, HDR, HDR_CONT = 0, 1, 2, 3                        # item kinds of the emulation


def test_the_abi_has_the_levels(wm):
    """Fails on a tree without the feature.  The field is the newest of wmbus_cfg: behind every older field and in front of the input
    stage's five, which existing tests pin as the struct's last; wmbus_line and wmbus_timing did not change."""
    assert [f[0] for f in wm.Cfg._fields_][-7:] == ["clock_waves", "line_levels", "input_rate_hz", "input_shift_hz", "input_dc", "input_format", "input_gain_q8"]
    assert dict((f[0], f[1]) for f in wm.Cfg._fields_)["line_levels"] is ctypes.c_uint
    assert [f[0] for f in wm.Line._fields_] == ["stream", "chain", "algo", "crc_ok", "pad", "sample", "text_off", "text_len"] and ctypes.sizeof(wm.Line) == 24
    assert [f[0] for f in wm.Timing._fields_][-2:] == ["input_bytes_out", "input_clipped"]
    assert [(f[0], ctypes.sizeof(f[1])) for f in wm.Level._fields_] == [("sync_sample", 8), ("offset_hz", 4), ("dev_hz", 4), ("n", 4), ("pad", 4)]
    assert ctypes.sizeof(wm.Level) == 24 == LEVEL_DTYPE.itemsize
    c = wm.Cfg()
    c.line_levels = 7
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.line_levels == 0
    for name in ("wmbus_line_levels", "wmbus_batch_line_levels"):
        assert name in wm.EXPORTS and hasattr(wm.lib(), name)
    assert hasattr(wm.Receiver, "line_levels")


# ---- the restatement by hand ---------------------------------------------------------------------------------------------------
def test_the_restatement_by_hand():
    q = LR.quantise(np.array([1.0, -1.0, 1.5, -7.0, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.5 / 2**20, 1.5 / 2**20, 2.5 / 2**20, -0.5 / 2**20, -1.5 / 2**20,
                              1e-30, 3.0 / 2**20], np.float32))
    assert q.tolist() == [2**20, -2**20, 2**20, -2**20, 2**20, -2**20, 0, 0, 0, 0, 2, 2, 0, -2, 0, 3]       # half to even
    # a constant 1/16 (25 kHz) in the T1/C1 window: sum = 128 x 65536, no deviation
    s = np.full(1000, 1 / 16, np.float32)
    assert LR.level(s, 256, 0) == dict(sync_sample=256, offset_hz=25000, dev_hz=0, n=128)
    assert LR.level(s, 255, 0) == dict(sync_sample=255, offset_hz=0, dev_hz=0, n=0)
    assert LR.level(s, 781, 1)["n"] == 0 and LR.level(-s, 782, 1) == dict(sync_sample=782, offset_hz=-25000, dev_hz=0, n=196)
    # +-1/8 alternating around -1/80 (-5 kHz): mean absolute deviation 50 kHz; floor division for the negative numerator
    s = (np.where(np.arange(1000) % 2 == 0, 1 / 8, -1 / 8) - 1 / 80).astype(np.float32)
    lv = LR.level(s, 500, 0)
    assert lv["offset_hz"] == -5000 and lv["dev_hz"] == 50000
    # the values only count inside [a - lo, a - hi)
    t = s.copy(); t[:500 - 256] = 9; t[500 - 128:] = -9
    assert LR.level(t, 500, 0) == lv
    t[500 - 256] = 9
    assert LR.level(t, 500, 0) != lv


# ---- the device source on the block emulator --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k3_levels.h", "wm_k2_common.h", "wm_dev.h")]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_lev_new.restype = ctypes.c_void_p
    L.wm_emu_lev_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_lev_push.restype = ctypes.c_long
    L.wm_emu_lev_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_uint32, ctypes.c_void_p]
    L.wm_emu_lev_read_tail.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.wm_emu_lev_record_bytes() == LEVEL_DTYPE.itemsize and L.wm_emu_lev_tail() == LR.TAIL
    return L


def soft_symbols(rng, n):
    """[2, n] float32: what a discriminator gives (|s| < 1, a preamble-like square wave with an offset in places) and what it hardly
    ever does -- +-1.0 exactly, values beyond +-1, infinities, NaN, and the ties of the rounding, (k + 1/2) / 2^20 for even and odd k."""
    s = rng.uniform(-0.3, 0.3, (2, n)).astype(np.float32)
    for ch in range(2):
        for start in rng.integers(0, max(1, n - 900), max(2, n // 3000)):
            k = np.arange(start, min(n, start + 900))
            s[ch, k] = (np.where((k // (4 if ch == 0 else 12)) % 2 == 0, 0.12, -0.12) + rng.uniform(-0.1, 0.1) + rng.normal(0, 0.01, k.size)).astype(np.float32)
        special = np.array([1.0, -1.0, 1.25, -3.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
        idx = rng.integers(0, n, max(8, n // 40))
        s[ch, idx] = special[rng.integers(0, special.size, idx.size)]
        idx = rng.integers(0, n, max(8, n // 20))
        s[ch, idx] = ((rng.integers(-2**20 - 3, 2**20 + 3, idx.size) + 0.5) / 2**20).astype(np.float32)         # exact in f32: 22 significant bits
    return s


def items_of_push(rng, m0, M, first):
    """(rel, chain, kind) of a push's items: random ones and, per chain, the directed ones -- the window wholly in the tail, straddling the
    push's start, wholly in the array, at both ends of the push, and (first push) in front of the stream."""
    out = []
    for ch in (0, 1):
        lo, hi = LR.LO[ch], LR.HI[ch]
        directed = [0, 1, hi - 1, hi, hi + 1, (lo + hi) // 2, lo - 1, lo, lo + 1, M - 1, M - 2, M // 2]
        for rel in directed + list(rng.integers(0, M, 24)):
            if 0 <= rel < M:
                out.append((int(rel), ch, int(rng.integers(0, 4))))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def run_pushes(emu, s, cuts, rng):
    """Every record the emulated kernels give over the pushes `cuts` (decimated samples each), with what level_ref says of it."""
    h = emu.wm_emu_lev_new()
    got = []
    try:
        m0 = 0
        for pi, M in enumerate(cuts):
            Mcap = (M + 255) // 256 * 256 + 256
            dphi = np.full((2, Mcap), 7e29, np.float32)          # beyond M: nothing a window may read
            dphi[:, :M] = s[:, m0:m0 + M]
            items = items_of_push(rng, m0, M, pi == 0)
            rel = np.array([i[0] for i in items], np.uint32); chain = np.array([i[1] for i in items], np.uint8); kind = np.array([i[2] for i in items], np.uint8)
            out = np.zeros(len(items), LEVEL_DTYPE)
            assert emu.wm_emu_lev_push(h, dphi.ctypes.data, M, Mcap, rel.ctypes.data, chain.ctypes.data, kind.ctypes.data, len(items), out.ctypes.data) == 0
            for (r, ch, kd), rec in zip(items, out):
                got.append((pi, m0 + r, ch, kd, rec))
            m0 += M
            # the carried tail: the last 782 soft symbols of the stream so far, zero in front of it
            tail = np.zeros((2, LR.TAIL), np.float32)
            emu.wm_emu_lev_read_tail(h, tail.ctypes.data)
            want = np.zeros((2, LR.TAIL), np.float32)
            k = min(m0, LR.TAIL)
            want[:, LR.TAIL - k:] = s[:, m0 - k:m0]
            assert np.array_equal(tail.view(np.uint32), want.view(np.uint32)), f"tail after push {pi}"
    finally:
        emu.wm_emu_lev_free(h)
    return got


def check(got, s):
    for pi, a, ch, kind, rec in got:
        assert rec["pad"] == 0
        if kind == HDR_CONT:                                   # measured in the push that held its access code: nothing here
            assert (rec["sync_sample"], rec["offset_hz"], rec["dev_hz"], rec["n"]) == (0, 0, 0, 0)
            continue
        want = LR.level(s[ch], a, ch)
        have = dict(sync_sample=int(rec["sync_sample"]), offset_hz=int(rec["offset_hz"]), dev_hz=int(rec["dev_hz"]), n=int(rec["n"]))
        assert have == want, (pi, a, ch, kind, have, want)


# pushes in bytes as the issue names them, and the decimation that turns them into samples
SEQUENCES = {"d2-uneven": ([4096 * 7, 4096 * 20, 4096, 4096 * 64], 2), "d16-4096": ([4096] * 24, 16)}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_emulated_kernels_give_the_restated_records(emu, name):
    nbytes, d = SEQUENCES[name]
    cuts = [b // 2 // d for b in nbytes]                       # 7168, 20480, 1024, 65536 | 128 each: shorter than the tail
    rng = np.random.default_rng(0x1E7E15 + d)
    s = soft_symbols(rng, sum(cuts))
    got = run_pushes(emu, s, cuts, rng)
    check(got, s)
    # every place a window can lie was met, in both chains
    for ch in (0, 1):
        lo, hi = LR.LO[ch], LR.HI[ch]
        starts = np.cumsum([0] + cuts[:-1])
        rel = [(a - starts[pi], a) for pi, a, c, kind, _ in got if c == ch and kind != HDR_CONT]
        assert any(a < lo for _, a in rel)                                        # in front of the stream
        assert any(r <= hi and a >= lo for r, a in rel)                           # wholly in the tail
        if max(cuts) > hi + 1:
            assert any(hi < r < lo and a >= lo for r, a in rel)                   # straddling
        if max(cuts) > lo:
            assert any(r >= lo for r, _ in rel)                                   # wholly in the array
    assert {kind for _, _, _, kind, _ in got} == {PKT_RLA, PKT_T2A, HDR, HDR_CONT}


def test_emulated_directed_windows(emu):
    """Windows made of the directed values alone: all +1.0 (the clamp's edge: 400 kHz), all beyond it, all NaN, all ties."""
    n = 4096
    rows = {"one": np.full(n, 1.0, np.float32), "beyond": np.full(n, -2.5, np.float32), "nan": np.full(n, np.nan, np.float32),
            "ties": ((np.arange(n) % 7 - 3 + 0.5) / 2**20).astype(np.float32), "inf": np.where(np.arange(n) % 2 == 0, np.inf, -np.inf).astype(np.float32)}
    rng = np.random.default_rng(5)
    for name, row in rows.items():
        s = np.stack([row, row])
        got = run_pushes(emu, s, [1024, 3072], rng)
        check(got, s)
    assert LR.level(rows["one"], 2000, 0)["offset_hz"] == 400000 and LR.level(rows["beyond"], 2000, 1)["offset_hz"] == -400000
    assert LR.level(rows["nan"], 2000, 0) == dict(sync_sample=2000, offset_hz=0, dev_hz=0, n=128)
    assert LR.level(rows["inf"], 2000, 0)["dev_hz"] == 400000


# ---- what the measurement is for: the oracle alone -----------------------------------------------------------------------------------
OFFSETS_KHZ = [0, 20, -35]
# Measured on the oracle's taps with level_ref (this test prints the figures): the worst |median - generator's offset| over the six
# captures below was MEASURED_WORST_HZ; the test allows twice that.  The generator draws every telegram's carrier
# from U(-10, +10) kHz around the offset, so single telegrams scatter by that much and the median over a capture's 40-70 clean
# telegrams by up to 2 kHz.
MEASURED_WORST_HZ = 1763                 # d = 2, +20 kHz: median 18237.5 Hz over 52 hits (d = 2, -35 kHz: 1595; d = 3, -35 kHz: 1714)
ALLOWED_HZ = 2 * MEASURED_WORST_HZ


def clean_sync_levels(wm, oracle, d, khz, seed=0x0FF5E7):
    """offset_hz of level_ref at the oracle's sync-flag chips that lead to CRC-clean lines: for every generated telegram whose payload a
    CRC-clean line of a framer prints, that framer's first sync-flag chip of the telegram's chain inside the telegram."""
    cu8, frames = wm.synth_capture(seed=seed + d, n_samples=(1 << 19) * d, fs_khz=800 * d, kinds=wm.T1 | wm.C1A | wm.C1B | wm.S1, frames_per_s=150.0,
                                   t1c1_center_khz=float(khz), s1_center_khz=float(khz))
    ref = oracle.run(cu8, oracle.make_opts(decimation=d), taps=True, chips=True)
    clean = {"rla": set(), "t2a": set()}
    for line in ref["text"].splitlines():
        f = line.split(";")
        if f[2] == "1":
            clean[f[0]].add(f[-1][2:].lower())
    out = []
    for fr in frames:
        ch = 1 if fr["kind"] == wm.S1 else 0
        for algo, tag in ((0, "rla"), (1, "t2a")):
            if not fr["complete"] or fr["telegram"].hex() not in clean[tag]:
                continue
            sync = LR.sync_chips(ref["chips"], ch, algo)
            inside = sync[(sync >= fr["start"] // d) & (sync < (fr["start"] + fr["n"]) // d + 64)]
            if inside.size:
                out.append((ch, LR.level(ref["dphi_fir"][ch], inside[0], ch)))
    return out


@pytest.mark.parametrize("d", [2, 3])
def test_median_offset_tracks_the_generator(wm, oracle, d):
    worst = 0
    for khz in OFFSETS_KHZ:
        levels = clean_sync_levels(wm, oracle, d, khz)
        assert len(levels) >= 40 and all(lv["n"] for _, lv in levels)
        off = np.array([lv["offset_hz"] for _, lv in levels])
        med = float(np.median(off))
        per_chain = [float(np.median([lv["offset_hz"] for c, lv in levels if c == ch])) for ch in (0, 1)]
        dev = float(np.median([lv["dev_hz"] for _, lv in levels]))
        print(f"d={d} offset {khz:+d} kHz: {len(levels)} hits, median {med:+.0f} Hz (T1/C1 {per_chain[0]:+.0f}, S1 {per_chain[1]:+.0f}), "
              f"single hits {off.min() - 1000 * khz:+d} ... {off.max() - 1000 * khz:+d} Hz around it, median dev_hz {dev:.0f}")
        worst = max(worst, abs(med - 1000 * khz))
        assert abs(med - 1000 * khz) <= ALLOWED_HZ, (d, khz, med)
    print(f"d={d}: worst |median - offset| {worst:.0f} Hz, allowed {ALLOWED_HZ}")
