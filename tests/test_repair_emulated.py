"""CRC repair (cfg.crc_repair): the device source of k3_repair (rtl-wmbus_amd/csrc/wm_k3_repair.h) on the coroutine block emulator,
behind the emulated k3_scan and k3_bursts, against the restatement tests/repair_ref.py on hand-made chip regions and soft-symbol rows:
every packet's flags, bytes and repair record.  No GPU needed.  Fails on a tree without the kernel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import level_ref as LR
import repair_ref as RR
import telegram_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "librepair_emu.so")
SRC = os.path.join(HERE, "emu", "repair_emu.cpp")
PKT = np.dtype([("stream", "<u4"), ("chain", "u1"), ("algo", "u1"), ("status", "u1"), ("flags", "u1"), ("chip0", "<u4"), ("consumed", "<u4"),
                ("sample", "<u8"), ("off", "<u4"), ("L", "<u2"), ("pkt_rssi", "u1"), ("rssi_now", "u1")])
REP = np.dtype([("blocks_bad", "<u2"), ("blocks_repaired", "<u2"), ("chips_flipped", "<u2"), ("pad", "<u2"), ("weight", "<u4")])
F_ALL = 8 | 16 | 32 | 64                                   # both chains, both framers
PKTF_C1, PKTF_B, PKTF_ERR36, PKTF_CRC = 1, 2, 4, 8
DONE, ABORT = 1, 2
SEG = 1024                                                  # samples per segment: 128 T1/C1 chips, 43 S1 chips -- telegrams span many segments
CAP = SEG // 4 + 8
STEP = {0: 8, 1: 24}                                        # samples per chip of the hand-made streams
STRONG = 0.12


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k3_repair.h", "wm_k3_levels.h", "wm_k3_bursts.h", "wm_k2_common.h", "wm_dev.h")]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_repair.restype = ctypes.c_long
    L.wm_emu_repair.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    assert L.wm_emu_rep_pkt_bytes() == PKT.itemsize and L.wm_emu_rep_record_bytes() == REP.itemsize == 12
    return L


def payload(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8))


def air_a(seed, lfield):
    return TR.frame_a(bytes([lfield]) + payload(seed, lfield))


def air_b(seed, total):
    return TR.frame_b(total, payload(seed, 300))


class Telegram:
    """One hand-made telegram: the chips of `air` in `mode` with the chips `flips` wrong (j counts from the access-code chip), and
    soft symbols that make the chips `weak` the least reliable, in that order; `offset` lifts every soft symbol of the telegram and its
    preamble (a carrier offset); ties: every chip equally reliable."""
    def __init__(self, mode, air, flips=(), weak=(), algo=1, offset=0.0, ties=False, gap=48):
        self.mode, self.air, self.flips, self.weak, self.algo, self.offset, self.ties, self.gap = mode, air, list(flips), list(weak), algo, offset, ties, gap
        self.chain = TR.CHAIN[mode]
        self.vals = TR.chips(mode, air)
        for j in self.flips:
            self.vals[j] ^= 1


class Push:
    """Telegrams laid one after the other into the chip regions of their (chain, framer), the soft symbols under them, and the stream in
    front of the push (m0 samples of it; the last 782 are the tail)."""
    def __init__(self, telegrams, m0=0, lead=40, seed=1):
        rng = np.random.default_rng(seed)
        self.m0, self.telegrams = m0, telegrams
        cursor = {(ch, al): lead for ch in (0, 1) for al in (0, 1)}        # next free sample of each chip stream
        index = {(ch, al): 0 for ch in (0, 1) for al in (0, 1)}
        self.chips = {k: [] for k in cursor}                              # (pos, value)
        soft = {0: {}, 1: {}}
        for t in telegrams:
            key = (t.chain, t.algo)
            step = STEP[t.chain]
            lo = LR.LO[t.chain]
            a = cursor[key]
            # the preamble in front of the access code: alternating around the offset, as far back as the push (and the stream) reaches
            for m in range(a - lo - 8, a):
                soft[t.chain][m] = (STRONG if (m // step) % 2 else -STRONG) + t.offset
            t.chip0, t.pos = index[key], a + step * np.arange(len(t.vals))
            amp = np.full(len(t.vals), STRONG) if t.ties else STRONG + rng.uniform(0.0, 0.05, len(t.vals))
            for rank, j in enumerate(t.weak):
                amp[j] = 0.002 * (rank + 1)
            for j, (p, v) in enumerate(zip(t.pos, t.vals)):
                self.chips[key].append((int(p), int(v)))
                if t.algo == 1:
                    soft[t.chain][int(p)] = (amp[j] if v & 1 else -amp[j]) + t.offset
            index[key] += len(t.vals)
            cursor[key] = int(t.pos[-1]) + step * t.gap
        self.M = (max(cursor.values()) + SEG - 1) // SEG * SEG
        self.Mcap = self.M + 256
        # the stream from its first sample on: noise in front of the push and between the telegrams
        self.s = rng.uniform(-0.05, 0.05, (2, m0 + self.M)).astype(np.float32)
        for ch in (0, 1):
            for m, v in soft[ch].items():
                if m + m0 >= 0:
                    self.s[ch, m + m0] = v
        nseg = self.M // SEG
        self.regions = [np.zeros((2, nseg, CAP), np.uint32) for _ in range(2)]
        self.counts = [np.zeros((2, nseg), np.uint32) for _ in range(2)]
        self.seen = [np.zeros((2, nseg), np.uint32) for _ in range(2)]
        for (ch, al), lst in self.chips.items():
            for p, v in lst:
                sg = p // SEG
                k = self.counts[al][ch, sg]
                self.regions[al][ch, sg, k] = ((p % SEG) << 3) | v
                self.counts[al][ch, sg] = k + 1
                if v & 2:
                    self.seen[al][ch, sg] = 1
        self.geo = np.array([self.M, self.Mcap, F_ALL, m0, SEG, SEG, nseg, nseg, CAP, CAP], np.uint64)

    def run(self, emu, repair=True, max_blocks=3):
        dphi = np.full((2, self.Mcap), 7e29, np.float32)              # beyond M: nothing the kernel may read
        dphi[:, :self.M] = self.s[:, self.m0:]
        tail = np.zeros((2, LR.TAIL), np.float32)
        k = min(self.m0, LR.TAIL)
        if k:
            tail[:, LR.TAIL - k:] = self.s[:, self.m0 - k:self.m0]
        rssi = np.full((2, self.Mcap), 40, np.uint8)
        cap = 64
        before, after, reps = np.zeros(cap, PKT), np.zeros(cap, PKT), np.zeros(cap, REP)
        bytes_before, arena = np.zeros(1 << 15, np.uint8), np.zeros(1 << 15, np.uint8)
        n = emu.wm_emu_repair(self.geo.ctypes.data, self.regions[0].ctypes.data, self.regions[1].ctypes.data, self.counts[0].ctypes.data,
                              self.counts[1].ctypes.data, self.seen[0].ctypes.data, self.seen[1].ctypes.data, rssi.ctypes.data, dphi.ctypes.data,
                              tail.ctypes.data, before.ctypes.data, bytes_before.ctypes.data, after.ctypes.data, cap, arena.ctypes.data, arena.size,
                              reps.ctypes.data, max_blocks, int(repair))
        assert n >= 0, n
        return before[:n], bytes_before, after[:n], arena, reps[:n]

    def check(self, emu):
        """Every packet of the push against the restatement; returns {telegram index: (result of the restatement or None, record, packet after)}."""
        before, bytes_before, after, arena, reps = self.run(emu)
        assert len(before) == len(self.telegrams)
        out = {}
        for ti, t in enumerate(self.telegrams):
            sel = np.nonzero((before["chain"] == t.chain) & (before["algo"] == t.algo) & (before["chip0"] == t.chip0))[0]
            assert sel.size == 1, (ti, before)
            i = int(sel[0])
            b, a, rec = before[i], after[i], reps[i]
            assert rec["pad"] == 0
            same = [n for n in PKT.names if n != "flags"]
            assert all(b[n] == a[n] for n in same), (ti, b, a)
            L, off = int(b["L"]), int(b["off"])
            subject = b["status"] == DONE and t.algo == 1 and not b["flags"] & PKTF_CRC and L >= 12
            res = None
            if subject:
                mode = "S1" if t.chain else "C1" if b["flags"] & PKTF_C1 else "T1"
                c = RR.preamble_mean(self.s[t.chain], self.m0 + int(t.pos[0]), t.chain)
                r = RR.reliabilities(self.s[t.chain], self.m0 + t.pos, c)
                res = RR.repair_telegram(mode, bool(b["flags"] & PKTF_B), L, np.asarray(t.vals), r)
                res["c"] = c
                want = res["record"]
            else:
                want = RR.ZERO
            have = {k: int(rec[k]) for k in want}
            assert have == want, (ti, have, want)
            if res and res["repaired"]:
                assert bytes(arena[off:off + L]) == res["air"], ti
                assert a["flags"] == (int(b["flags"]) & ~PKTF_ERR36) | PKTF_CRC | (PKTF_ERR36 if res["err3of6"] else 0), ti
            else:
                assert a["flags"] == b["flags"], ti
                assert bytes(arena[off:off + max(L, 2)]) == bytes(bytes_before[off:off + max(L, 2)]), ti
            out[ti] = (res, have, a)
        # nothing outside the packets' own slots of the arena changed
        mask = np.ones(arena.size, bool)
        for b in before:
            if b["status"] == DONE:
                mask[int(b["off"]):int(b["off"]) + int(b["L"])] = False
        assert np.array_equal(arena[mask], bytes_before[mask])
        return out


def chip_of(mode, byte, k=0):
    """Chip j of chip k of telegram byte `byte`."""
    return RR.OFF[mode] + RR.CPB[mode] * byte + k


def test_ties_resolve_by_chip_index(emu):
    """Equal reliabilities: the candidates are the block's first eight chips (behind the L-field's in the first block)."""
    tg = [Telegram("C1A", air_a(1, 40), flips=[chip_of("C1", 12, 5)], ties=True),          # second block: chips of byte 12, the sixth of them wrong
          Telegram("C1A", air_a(2, 40), flips=[chip_of("C1", 13, 0)], ties=True),          # the ninth chip of the block: out of reach
          Telegram("C1A", air_a(3, 40), flips=[chip_of("C1", 1, 7)], ties=True)]           # first block: the candidates begin behind the L-field
    got = Push(tg).check(emu)
    assert got[0][1] == dict(blocks_bad=1, blocks_repaired=1, chips_flipped=1, weight=got[0][1]["weight"]) and got[0][0]["air"] == tg[0].air
    assert got[1][1]["blocks_bad"] == 1 and got[1][1]["blocks_repaired"] == 0
    assert got[2][1]["blocks_repaired"] == 1 and got[2][0]["air"] == tg[2].air


def test_the_l_field_is_never_flipped(emu):
    """A first block whose L-field chips are the least reliable of all: no candidate among them, the error behind them is found."""
    for mode, name in (("T1", "T1"), ("C1A", "C1"), ("S1", "S1")):
        lf = [chip_of(name, 0, k) for k in range(RR.CPB[name])]
        err = [chip_of(name, 5, 2)] + ([chip_of(name, 5, 3)] if mode == "S1" else [])       # S1: both chips of a pair
        tg = [Telegram(mode, air_a(4, 25), flips=err, weak=lf + err)]
        got = Push(tg).check(emu)
        res, rec, _ = got[0]
        assert rec["blocks_repaired"] == 1 and res["air"] == tg[0].air, mode


def test_only_a_three_chip_pattern_is_valid(emu):
    wrong = [chip_of("C1", 14, 1), chip_of("C1", 20, 6), chip_of("C1", 27, 3)]
    others = [chip_of("C1", 13, 0), chip_of("C1", 16, 4), chip_of("C1", 22, 2)]
    tg = [Telegram("C1A", air_a(5, 40), flips=wrong, weak=[others[0], wrong[0], others[1], wrong[1], others[2], wrong[2]])]
    res, rec, _ = Push(tg).check(emu)[0]
    assert (rec["blocks_bad"], rec["blocks_repaired"], rec["chips_flipped"]) == (1, 1, 3) and res["air"] == tg[0].air


def test_two_bad_blocks_one_unrepairable_changes_nothing(emu):
    """All or nothing: the record reports the block that has a repair, the line's bytes and flags stay."""
    good, lost = chip_of("T1", 14, 3), [chip_of("T1", 33, k) for k in (0, 4, 7, 9)]       # four strong chips of one byte wrong: out of reach
    tg = [Telegram("T1", air_a(6, 40), flips=[good] + lost, weak=[good]),
          Telegram("T1", air_a(7, 40), flips=[good, chip_of("T1", 33, 2)], weak=[good, chip_of("T1", 33, 2)])]      # both blocks within reach
    got = Push(tg).check(emu)
    assert (got[0][1]["blocks_bad"], got[0][1]["blocks_repaired"]) == (2, 1) and not got[0][0]["repaired"]
    assert (got[1][1]["blocks_bad"], got[1][1]["blocks_repaired"], got[1][1]["chips_flipped"]) == (2, 2, 2) and got[1][0]["air"] == tg[1].air


def test_short_last_blocks(emu):
    """A last block of two bytes is clean only as 0xFFFF and, bad, has no repair; one of three bytes has."""
    b130, b131, a15 = air_b(8, 130), air_b(9, 131), air_a(10, 10)
    assert b130[-2:] == b"\xff\xff" and len(a15) == 15
    e2, e3 = chip_of("C1", 129, 4), chip_of("C1", 130, 4)
    tg = [Telegram("C1B", b130, flips=[e2], weak=[e2]),                                     # the error in the two-byte block
          Telegram("C1B", b130, flips=[chip_of("C1", 60, 1)], weak=[chip_of("C1", 60, 1)]),  # the error in the 128-byte block, 0xFFFF behind it
          Telegram("C1B", b131, flips=[e3], weak=[e3]),
          Telegram("T1", a15, flips=[chip_of("T1", 13, 5)], weak=[chip_of("T1", 13, 5)])]
    got = Push(tg).check(emu)
    assert (got[0][1]["blocks_bad"], got[0][1]["blocks_repaired"]) == (1, 0)
    for ti in (1, 2, 3):
        assert got[ti][1]["blocks_repaired"] == 1 and got[ti][0]["air"] == tg[ti].air, ti


def test_frame_b_block_of_1024_chips(emu):
    """128 bytes of NRZ are 1024 chips: sixteen trips of the wave, the weak chips spread over them."""
    air = air_b(11, 256)
    wrong = [chip_of("C1", 3, 0), chip_of("C1", 126, 7)]
    weak = [chip_of("C1", 40, 3), wrong[0], chip_of("C1", 77, 7), chip_of("C1", 100, 1), wrong[1], chip_of("C1", 127, 7), chip_of("C1", 1, 0)]
    tg = [Telegram("C1B", air, flips=wrong + [chip_of("C1", 200, 2)], weak=weak + [chip_of("C1", 200, 2)])]
    res, rec, _ = Push(tg).check(emu)[0]
    assert (rec["blocks_bad"], rec["blocks_repaired"], rec["chips_flipped"]) == (2, 2, 3) and res["air"] == air


def test_window_in_front_of_the_stream_and_in_the_tail(emu):
    """c = 0 where the preamble window would begin before the stream's first sample; a window that lies in the carried tail is read
    from there.  With a carrier offset of 0.06 the order of the reliabilities depends on c: the restatement must see the same one."""
    def telegram():
        e = chip_of("T1", 20, 1)
        t = Telegram("T1", air_a(12, 40), flips=[e], offset=0.06)
        t.weak = [e]
        return t
    early = Push([telegram()], m0=0, lead=40)
    res, rec, _ = early.check(emu)[0]
    assert res["c"] == 0 and rec["blocks_bad"] == 1
    for m0, lead in ((5000, 40), (300, 100), (7 * 1024, 200)):                 # wholly in the tail; the tail shorter than 782; straddling
        late = Push([telegram()], m0=m0, lead=lead)
        res, rec, _ = late.check(emu)[0]
        assert abs(res["c"] - round(0.06 * 2**20)) < 2**13 and rec["blocks_bad"] == 1, (m0, res["c"])
        assert rec["blocks_repaired"] == 1                                        # the weak chip lies at the offset itself: the least reliable with the true c


def test_line_codes(emu):
    """T1: a block with an invalid symbol; one where flipping the least reliable chip alone makes another symbol invalid, so the repair is
    the next pattern.  S1: a double error in one pair (a single one never completes the telegram)."""
    air = air_a(13, 40)
    e = chip_of("T1", 15, 2)
    vals = TR.chips("T1", air)
    sym = int("".join(str(v) for v in vals[chip_of("T1", 15, 0):chip_of("T1", 15, 6)]), 2)
    assert sym ^ (1 << 3) not in TR.NIBBLE_OF_SYMBOL                          # one wrong chip of a 3-out-of-6 symbol: never a code word
    decoy = chip_of("T1", 22, 4)                                             # a correct chip, less reliable than the wrong one
    tg = [Telegram("T1", air, flips=[e], weak=[e]),
          Telegram("T1", air, flips=[e], weak=[decoy, e]),
          Telegram("S1", air_a(14, 30), flips=[chip_of("S1", 17, 6), chip_of("S1", 17, 7)], weak=[chip_of("S1", 17, 7), chip_of("S1", 17, 6)])]
    got = Push(tg).check(emu)
    assert got[0][2]["flags"] & PKTF_CRC and not got[0][2]["flags"] & PKTF_ERR36 and got[0][1]["chips_flipped"] == 1
    assert got[1][1]["chips_flipped"] == 1 and got[1][0]["air"] == air         # m = 2, not m = 1 or 3
    assert got[2][1] == dict(blocks_bad=1, blocks_repaired=1, chips_flipped=2, weight=got[2][1]["weight"]) and got[2][0]["air"] == tg[2].air


def test_other_packets_are_untouched(emu):
    """A run-length packet with a bad CRC, a clean time2 packet, a time2 decoder that gave up: records of zeros, nothing changes."""
    e = chip_of("T1", 15, 2)
    tg = [Telegram("T1", air_a(15, 40), flips=[e], weak=[e], algo=0),
          Telegram("T1", air_a(16, 40)),
          Telegram("S1", air_a(17, 20), flips=[chip_of("S1", 9, 3)]),
          Telegram("T1", air_a(18, 40), flips=[e], weak=[e])]
    p = Push(tg)
    got = p.check(emu)
    before, _, after, _, reps = p.run(emu)
    assert sorted(before["status"].tolist()) == [DONE, DONE, DONE, ABORT]
    assert [got[i][1] for i in (0, 1, 2)] == [RR.ZERO] * 3 and got[3][1]["blocks_repaired"] == 1
    # without the kernel the packets are k3_bursts' own
    plain, _, same, _, _ = p.run(emu, repair=False)
    assert np.array_equal(plain, same) and np.array_equal(plain, before)
