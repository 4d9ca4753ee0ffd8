"""Line quality (cfg.line_quality): the device source of k3_quality (rtl-wmbus_amd/csrc/wm_k3_quality.h) on the coroutine block
emulator, behind the emulated k3_scan and k3_bursts, against the restatement tests/quality_ref.py on hand-made chip regions and
soft-symbol rows: every packet's record, and that packets and bytes stay as they were.  No GPU needed.  Fails on a tree without the
kernel."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import quality_ref as QR
import repair_ref as RR
import telegram_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libquality_emu.so")
SRC = os.path.join(HERE, "emu", "quality_emu.cpp")
PKT = np.dtype([("stream", "<u4"), ("chain", "u1"), ("algo", "u1"), ("status", "u1"), ("flags", "u1"), ("chip0", "<u4"), ("consumed", "<u4"),
                ("sample", "<u8"), ("off", "<u4"), ("L", "<u2"), ("pkt_rssi", "u1"), ("rssi_now", "u1")])
REC = np.dtype([("n", "<u4"), ("chip_rate_chz", "<u4"), ("jitter_ns", "<u4"), ("hi_hz", "<i4"), ("lo_hz", "<i4"), ("spread_hz", "<u4"), ("eye_hz", "<i4"),
                ("pad", "<u4")])
F_ALL = 8 | 16 | 32 | 64                                   # both chains, both framers
PKTF_C1 = 1
DONE, ABORT = 1, 2
SEG = 1024                                                  # samples per segment: 128 T1/C1 chips, 43 S1 chips -- telegrams span many segments
CAP = SEG // 4 + 8
STEP = {0: Fraction(8), 1: Fraction(24)}                    # nominal samples per chip of the hand-made streams
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k3_quality.h", "wm_k3_repair.h", "wm_k3_levels.h", "wm_k3_bursts.h",
                                                                                             "wm_k2_common.h", "wm_dev.h")]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_quality.restype = ctypes.c_long
    L.wm_emu_quality.argtypes = [ctypes.c_void_p] * 12 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    assert L.wm_emu_q_pkt_bytes() == PKT.itemsize and L.wm_emu_q_record_bytes() == REC.itemsize == 32
    return L


def rate_tol(nominal_chz, n, step):
    """Positions are floor(step j): each is up to one sample early.  A perturbation within a band of 1 sample moves a least-squares slope
    by at most 0.5 sum |j - mean| / sum (j - mean)^2 < 1.5 / n samples per chip; one unit for the rounding."""
    return nominal_chz * Fraction(3, 2 * n) / Fraction(step) + 1


def payload(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8))


def air_a(seed, lfield):
    return TR.frame_a(bytes([lfield]) + payload(seed, lfield))


class Telegram:
    """One hand-made telegram: the chips of `air` in `mode`, chip j at sample a + floor(step j) (+ `slip` samples from chip `slip_at`
    on), a soft symbol of +-amp (+ a little per-chip variation) + offset under every chip, negated for `invert`, and for the chips in
    `wrong` a weak symbol of the other sign.  `flips`: chips that are wrong in the chip stream itself.  start: the access-code chip's
    sample (None: behind the telegram before)."""
    def __init__(self, mode, air, algo=1, step=None, slip_at=None, slip=0, amp=0.12, vary=0.03, offset=0.0, invert=False, wrong=(), flips=(), start=None, gap=48):
        self.mode, self.air, self.algo, self.chain = mode, air, algo, TR.CHAIN[mode]
        self.step = Fraction(step) if step is not None else STEP[self.chain]
        self.slip_at, self.slip, self.amp, self.vary, self.offset, self.invert, self.wrong, self.start, self.gap = slip_at, slip, amp, vary, offset, invert, set(wrong), start, gap
        self.vals = TR.chips(mode, air)
        for j in flips:
            self.vals[j] ^= 1

    def positions(self, a):
        pos = np.array([a + int(self.step * j) for j in range(len(self.vals))], np.int64)
        if self.slip_at is not None:
            pos[self.slip_at:] += self.slip
        return pos


class Push:
    def __init__(self, telegrams, m0=0, lead=40, seed=1, M=None):
        rng = np.random.default_rng(seed)
        self.m0, self.telegrams = m0, telegrams
        cursor = {0: lead, 1: lead}                                       # next free sample of each chain's row
        index = {(ch, al): 0 for ch in (0, 1) for al in (0, 1)}
        chips = {k: [] for k in index}
        soft = {0: {}, 1: {}}
        for t in telegrams:
            a = cursor[t.chain] if t.start is None else t.start
            assert a >= cursor[t.chain] or t.start is None
            t.chip0, t.pos = index[(t.chain, t.algo)], t.positions(a)
            amp = t.amp + rng.uniform(0.0, t.vary, len(t.vals)) if t.vary else np.full(len(t.vals), t.amp)
            for j, (p, v) in enumerate(zip(t.pos, t.vals)):
                chips[(t.chain, t.algo)].append((int(p), int(v)))
                s = amp[j] if v & 1 else -amp[j]
                if j in t.wrong:
                    s = -0.01 if v & 1 else 0.01
                soft[t.chain][int(p)] = (-s if t.invert else s) + t.offset
            index[(t.chain, t.algo)] += len(t.vals)
            cursor[t.chain] = int(t.pos[-1]) + int(STEP[t.chain]) * t.gap
        full = (max(cursor.values()) + SEG - 1) // SEG * SEG
        self.M = full if M is None else M
        assert self.M % SEG == 0
        self.Mcap = self.M + 256
        self.s = rng.uniform(-0.05, 0.05, (2, max(full, self.M))).astype(np.float32)
        for ch in (0, 1):
            for m, v in soft[ch].items():
                self.s[ch, m] = v
        nseg = self.M // SEG
        self.regions = [np.zeros((2, nseg, CAP), np.uint32) for _ in range(2)]
        self.counts = [np.zeros((2, nseg), np.uint32) for _ in range(2)]
        self.seen = [np.zeros((2, nseg), np.uint32) for _ in range(2)]
        for (ch, al), lst in chips.items():
            for p, v in lst:
                if p >= self.M:
                    continue                                              # beyond the push
                sg = p // SEG
                k = self.counts[al][ch, sg]
                self.regions[al][ch, sg, k] = ((p % SEG) << 3) | v
                self.counts[al][ch, sg] = k + 1
                if v & 2:
                    self.seen[al][ch, sg] = 1
        self.geo = np.array([self.M, self.Mcap, F_ALL, m0, SEG, SEG, nseg, nseg, CAP, CAP], np.uint64)

    def run(self, emu, max_blocks=3, patch=(NONE, 0)):
        dphi = np.full((2, self.Mcap), 7e29, np.float32)              # beyond M: nothing the kernel may read
        dphi[:, :self.M] = self.s[:, :self.M]
        rssi = np.full((2, self.Mcap), 40, np.uint8)
        cap = 64
        before, after, recs = np.zeros(cap, PKT), np.zeros(cap, PKT), np.zeros(cap, REC)
        bytes_before, arena = np.zeros(1 << 15, np.uint8), np.zeros(1 << 15, np.uint8)
        n = emu.wm_emu_quality(self.geo.ctypes.data, self.regions[0].ctypes.data, self.regions[1].ctypes.data, self.counts[0].ctypes.data,
                               self.counts[1].ctypes.data, self.seen[0].ctypes.data, self.seen[1].ctypes.data, rssi.ctypes.data, dphi.ctypes.data,
                               before.ctypes.data, bytes_before.ctypes.data, after.ctypes.data, cap, arena.ctypes.data, arena.size,
                               recs.ctypes.data, max_blocks, patch[0], patch[1])
        assert n >= 0, n
        assert np.array_equal(before[:n], after[:n]) and np.array_equal(bytes_before, arena)      # the kernel writes its records, nothing else
        return before[:n], recs[:n]

    def slot(self, pkts, t):
        sel = np.nonzero((pkts["chain"] == t.chain) & (pkts["algo"] == t.algo) & (pkts["chip0"] == t.chip0))[0]
        return int(sel[0]) if sel.size == 1 else None

    def check(self, emu, expect_pkts=None, **kw):
        """Every packet of the push against the restatement; returns [record dict or None (no packet) per telegram]."""
        pkts, recs = self.run(emu, **kw)
        assert len(pkts) == (len(self.telegrams) if expect_pkts is None else expect_pkts)
        out = []
        for ti, t in enumerate(self.telegrams):
            i = self.slot(pkts, t)
            if i is None:
                out.append(None)
                continue
            b, rec = pkts[i], recs[i]
            assert rec["pad"] == 0
            want = QR.ZERO
            if b["status"] == DONE and t.algo == 1 and int(b["L"]) <= QR.MAX_BYTES:
                mode = "S1" if t.chain else "C1" if b["flags"] & PKTF_C1 else "T1"
                n = RR.OFF[mode] + RR.CPB[mode] * int(b["L"])
                assert n <= len(t.vals)
                want = QR.quality(t.pos[:n], np.asarray(t.vals[:n]), self.s[t.chain])
            have = {k: int(rec[k]) for k in QR.FIELDS}
            assert have == want, (ti, have, want)
            out.append(have)
        return out


def test_t1_of_twelve_bytes(emu):
    """n = 145: two full trips of the lanes and a partial one."""
    got = Push([Telegram("T1", air_a(1, 9))]).check(emu)
    assert got[0]["n"] == 145 and got[0]["chip_rate_chz"] == 10_000_000 and got[0]["jitter_ns"] == 0 and got[0]["eye_hz"] > 40000


def test_c1_and_s1(emu):
    got = Push([Telegram("C1A", air_a(2, 30)), Telegram("C1B", TR.frame_b(131, payload(3, 300))), Telegram("S1", air_a(4, 20), step=Fraction(3125, 128))]).check(emu)
    assert [g["n"] for g in got] == [17 + 8 * TR.frame_a_length(30), 17 + 8 * 131, 1 + 16 * TR.frame_a_length(20)]
    assert got[0]["chip_rate_chz"] == 10_000_000 and abs(got[2]["chip_rate_chz"] - 3_276_800) <= rate_tol(3_276_800, got[2]["n"], Fraction(3125, 128)) and 100 < got[2]["jitter_ns"] < 625


def test_segment_edges(emu):
    """The access-code chip as the last chip of its segment; a telegram over five segments; one whose first segment holds other chips
    in front of it."""
    tg = [Telegram("T1", air_a(5, 9), start=SEG - 1), Telegram("T1", air_a(6, 40), start=3 * SEG + 100, gap=4), Telegram("T1", air_a(7, 9))]
    p = Push(tg)
    assert tg[1].pos[564] // SEG - tg[1].pos[0] // SEG == 4 and tg[2].pos[0] // SEG == tg[1].pos[-1] // SEG
    got = p.check(emu)
    assert [g["n"] for g in got] == [145, 565, 145]


def test_longest_s1_with_symbols_at_the_clamp(emu):
    """n = 4673 = 1 + 16 x 292.  The longest telegram the decoder completes has 290 bytes; its chips and the 32 chips of idle tail
    behind them are 4673, so the packet's L is set to 292 behind k3_bursts.  +-3.0 quantises to +-2^20: S1 passes 2^31."""
    t = Telegram("S1", air_a(8, 255), amp=3.0, vary=0.0)
    assert len(t.vals) == 4673
    p = Push([t])
    got = p.check(emu, patch=(0, 292))
    assert got[0]["n"] == 4673 and (got[0]["hi_hz"], got[0]["lo_hz"], got[0]["spread_hz"], got[0]["eye_hz"]) == (400000, -400000, 0, 400000)
    assert got[0]["chip_rate_chz"] == 3_333_333
    assert p.check(emu)[0]["n"] == 1 + 16 * 290                           # and as the decoder left it


def test_chip_clocks_off_nominal_and_a_slip(emu):
    tg = [Telegram("T1", air_a(9, 40), step=Fraction(80, 11)), Telegram("T1", air_a(10, 40), step=Fraction(80, 9)),
          Telegram("C1A", air_a(11, 40), slip_at=200, slip=8), Telegram("S1", air_a(12, 12), step=Fraction(22), slip_at=100, slip=-5)]
    got = Push(tg).check(emu)
    assert abs(got[0]["chip_rate_chz"] - 11_000_000) <= rate_tol(11_000_000, got[0]["n"], Fraction(80, 11))
    assert abs(got[1]["chip_rate_chz"] - 9_000_000) <= rate_tol(9_000_000, got[1]["n"], Fraction(80, 9))
    assert got[0]["jitter_ns"] > 100 and got[2]["jitter_ns"] > 1500 and got[2]["chip_rate_chz"] < 10_000_000


def test_eye_corners(emu):
    """Inverted polarity; a chip on the wrong side; a carrier offset that lifts both levels above zero."""
    tg = [Telegram("T1", air_a(13, 20), invert=True), Telegram("T1", air_a(14, 20), wrong=[77]), Telegram("C1A", air_a(15, 20), offset=0.2),
          Telegram("S1", air_a(16, 10), invert=True, wrong=[5, 90], offset=-0.3)]
    got = Push(tg).check(emu)
    assert got[0]["hi_hz"] < 0 < got[0]["lo_hz"] and got[0]["eye_hz"] > 40000
    assert got[1]["eye_hz"] < 0 < got[1]["hi_hz"]
    assert got[2]["lo_hz"] > 0 and got[2]["eye_hz"] > 40000
    assert got[3]["eye_hz"] < 0 and got[3]["hi_hz"] < got[3]["lo_hz"] < 0


def test_push_behind_the_first(emu):
    """m0 > 0: positions are push-relative, the record is the one of the first push."""
    def tg():
        return [Telegram("T1", air_a(17, 25), step=Fraction(81, 10)), Telegram("S1", air_a(18, 10))]
    assert Push(tg(), m0=7 * SEG + 0).check(emu) == Push(tg()).check(emu)


def test_several_telegrams_per_wave(emu):
    """One block: four waves over eleven packets, subjects and others in turn."""
    tg = [Telegram("T1", air_a(20 + i, 9 + i), step=Fraction(8) + Fraction(i, 40), algo=int(i % 3 != 2)) for i in range(9)] + \
         [Telegram("S1", air_a(30, 9)), Telegram("S1", air_a(31, 12), invert=True)]
    got = Push(tg).check(emu, max_blocks=1)
    assert [g["n"] > 0 for g in got] == [i % 3 != 2 for i in range(9)] + [True, True]


def test_non_subjects(emu):
    """A run-length packet, a decoder that gave up (one wrong chip of a Manchester pair), a length beyond WM_PKT_MAXBYTES (set behind
    k3_bursts), a telegram whose chips run past the push (no packet at all: it travels as chips): n = 0, and nothing else changes."""
    tg = [Telegram("T1", air_a(40, 30), algo=0), Telegram("S1", air_a(41, 20), flips=[1 + 16 * 9 + 3]), Telegram("T1", air_a(42, 20)),
          Telegram("T1", air_a(43, 20)), Telegram("T1", air_a(44, 60))]
    full = Push(tg)
    M = int(tg[4].pos[300]) // SEG * SEG
    assert tg[4].pos[0] < M < tg[4].pos[-33] and tg[3].pos[-1] < M
    p = Push(tg, M=M)
    pkts, _ = p.run(emu)
    assert sorted(pkts["status"].tolist()) == [DONE, DONE, DONE, ABORT]
    got = p.check(emu, expect_pkts=4, patch=(p.slot(pkts, tg[2]), 293))
    assert got[:3] == [QR.ZERO] * 3 and got[3]["n"] == 1 + 12 * TR.frame_a_length(20) and got[4] is None
    assert full.check(emu)[2]["n"] == got[3]["n"]                         # the patched one is a subject as the decoder left it
