"""S1 rescue (cfg.s1_rescue): the device source of k3_rescue (rtl-wmbus_amd/csrc/wm_k3_rescue.h) on the coroutine block emulator, behind
the emulated k3_scan and k3_bursts, against the restatement tests/rescue_ref.py on hand-made chip regions, soft-symbol rows and RSSI
rows: every packet record, the byte arena and its counter, every rescue record.  No GPU needed.  Fails on a tree without the kernel.

The chip regions are laid out by test_repair_emulated.Push (telegrams one after the other, 24 samples per S1 chip, segments of 1024
samples); this file adds designed soft symbols and RSSI bytes under single chips."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import level_ref as LR
import rescue_ref as RF
import telegram_ref as TR
from test_repair_emulated import ABORT, CSRC, DONE, HERE, PKT, PKTF_CRC, Push, Telegram, air_a

SO = os.path.join(HERE, "emu", "librescue_emu.so")
SRC = os.path.join(HERE, "emu", "rescue_emu.cpp")
REC = np.dtype([("status", "<u2"), ("pairs", "<u2"), ("min_margin", "<u4"), ("blocks", "<u2"), ("pad", "<u2")])
PKTF_RESCUED = 16
WEAK = 0.01                                                # a chip received wrong, and barely: the pair's other chip decides


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k3_rescue.h", "wm_k3_repair.h", "wm_k3_levels.h", "wm_k3_bursts.h", "wm_k2_common.h", "wm_dev.h")]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_rescue.restype = ctypes.c_long
    L.wm_emu_rescue.argtypes = [ctypes.c_void_p] * 12 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    assert L.wm_emu_res_pkt_bytes() == PKT.itemsize and L.wm_emu_res_record_bytes() == REC.itemsize == 12
    assert L.wm_emu_res_lds_bytes() <= 4 * 1024                 # a block of four waves: about 1 KB a wave at the most
    return L


def pair_chips(i):
    """The two chips of data pair i (pair 0 is the L-field's first)."""
    return 1 + 2 * i, 2 + 2 * i


def s1(seed, lfield, wrong=(), **kw):
    """An S1 telegram with the chips `wrong` received wrong."""
    return Telegram("S1", air_a(seed, lfield), flips=list(wrong), **kw)


class RPush(Push):
    """test_repair_emulated.Push with designed soft symbols and RSSI bytes under single chips: soft / rssi = {(telegram, chip j): value}.
    A chip in `wrong` that has no entry in `soft` gets a WEAK soft symbol of its received sign, so that the pair's other chip decides --
    rightly."""
    def __init__(self, telegrams, soft=None, rssi=None, **kw):
        super().__init__(telegrams, **kw)
        self.rssi = np.full((2, self.Mcap), 40, np.uint8)
        soft = dict(soft or {})
        for ti, t in enumerate(telegrams):
            for j in t.flips:
                soft.setdefault((ti, j), WEAK if t.vals[j] & 1 else -WEAK)
        for (ti, j), v in soft.items():
            t = telegrams[ti]
            self.s[t.chain, self.m0 + int(t.pos[j])] = v
        for (ti, j), v in (rssi or {}).items():
            t = telegrams[ti]
            self.rssi[t.chain, int(t.pos[j])] = v

    def run(self, emu, bytes_cap=1 << 15, max_blocks=3):
        dphi = np.full((2, self.Mcap), 7e29, np.float32)              # beyond M: nothing the kernel may read
        dphi[:, :self.M] = self.s[:, self.m0:]
        cap = 64
        before, after, recs = np.zeros(cap, PKT), np.zeros(cap, PKT), np.zeros(cap, REC)
        bytes_before, arena = np.zeros(bytes_cap, np.uint8), np.zeros(bytes_cap, np.uint8)
        counters = np.zeros(3, np.uint32)
        n = emu.wm_emu_rescue(self.geo.ctypes.data, self.regions[0].ctypes.data, self.regions[1].ctypes.data, self.counts[0].ctypes.data,
                              self.counts[1].ctypes.data, self.seen[0].ctypes.data, self.seen[1].ctypes.data, self.rssi.ctypes.data, dphi.ctypes.data,
                              before.ctypes.data, bytes_before.ctypes.data, after.ctypes.data, cap, arena.ctypes.data, bytes_cap,
                              recs.ctypes.data, counters.ctypes.data, max_blocks)
        assert n >= 0, n
        assert counters[2] == n + 2                                   # the packet counter is only read
        return before[:n], bytes_before, after[:n], arena, recs[:n], counters

    def check(self, emu, bytes_cap=1 << 15, max_blocks=3):
        """Every packet of the push against the restatement; returns {telegram index: (kind, record, packet before, packet after)}."""
        before, bytes_before, after, arena, recs, counters = self.run(emu, bytes_cap, max_blocks)
        assert len(before) == len(self.telegrams)
        out, taken, claimed = {}, 0, np.zeros(bytes_cap, bool)
        for ti, t in enumerate(self.telegrams):
            sel = np.nonzero((before["chain"] == t.chain) & (before["algo"] == t.algo) & (before["chip0"] == t.chip0))[0]
            assert sel.size == 1, (ti, before)
            i = int(sel[0])
            b, a, rec = before[i], after[i], recs[i]
            assert rec["pad"] == 0
            kind, res = "no", None
            if b["status"] == ABORT and t.chain == 1 and t.algo == 1:
                rs = self.rssi[1, t.pos]
                kind, L = RF.examine(np.asarray(t.vals), rs, int(b["consumed"]))
                assert kind != "short"
                if kind == "subject":
                    assert L == b["L"]
                    n = 1 + 16 * L
                    q = LR.quantise(self.s[1, self.m0 + t.pos[1:n]])
                    res = RF.rescue_telegram(L, np.asarray(t.vals[1:n]) & 1, q)
            want = res["record"] if res else RF.ZERO
            have = {k: int(rec[k]) for k in want}
            room = True
            if res and res["rescued"] and not a["flags"] & PKTF_RESCUED:          # the arena had no room: status 3, everything else as computed
                assert have == dict(want, status=3), (ti, have, want)
                room = False
            else:
                assert have == want, (ti, have, want)
            # status and consumed, and whatever else identifies the burst, never change
            for name in ("stream", "chain", "algo", "status", "chip0", "consumed", "L", "pkt_rssi"):
                assert b[name] == a[name], (ti, name, b, a)
            if res and res["rescued"] and room:
                L, off, n = int(b["L"]), int(a["off"]), 1 + 16 * int(b["L"])
                assert a["flags"] == int(b["flags"]) | PKTF_CRC | PKTF_RESCUED, ti
                assert a["sample"] == self.m0 + int(t.pos[n - 1]) and a["rssi_now"] == self.rssi[1, int(t.pos[n - 1])], ti
                assert off % 4 == 0 and counters[0] <= off and off + L <= min(int(counters[1]), bytes_cap) and not claimed[off:off + L].any(), ti
                assert bytes(arena[off:off + L]) == res["air"], ti
                claimed[off:off + L] = True
                taken += (L + 3) & ~3
            else:
                assert a == b, (ti, b, a)
            out[ti] = (kind, have, b, a)
        # nothing outside the rescued telegrams' own slots of the arena changed
        assert np.array_equal(arena[~claimed], bytes_before[~claimed])
        return out, counters, taken


def test_first_pair_last_pair_and_the_trip_boundary(emu):
    """One chip wrong in the first pair of the data, in the last pair, and in pair 31 -- chips 63 and 64, the two sides of a 64-chip trip
    counted from the access-code chip: the lane layout keeps them in one trip.  Then all of them in one telegram."""
    L = TR.frame_a_length(40)
    last = 8 * L - 1
    cases = [[pair_chips(8)[0]], [pair_chips(8)[1]], [pair_chips(last)[0]], [pair_chips(last)[1]], [pair_chips(31)[0]], [pair_chips(31)[1]], [pair_chips(63)[1]],
             [pair_chips(8)[0], pair_chips(31)[1], pair_chips(32)[0], pair_chips(63)[0], pair_chips(64)[1], pair_chips(last)[1]]]
    tg = [s1(20 + k, 40, wrong) for k, wrong in enumerate(cases)]
    got, _, _ = RPush(tg).check(emu)
    for ti, wrong in enumerate(cases):
        kind, rec, b, a = got[ti]
        assert kind == "subject" and rec["status"] == 1 and rec["pairs"] == len(wrong) and rec["blocks"] == 3, (ti, rec)
        assert b["consumed"] == 2 * ((min(wrong) - 1) // 2) + 3 and rec["min_margin"] > 0


def test_several_invalid_pairs_in_one_block(emu):
    wrong = [pair_chips(i)[i & 1] for i in range(8 * 12, 8 * 12 + 40, 3)]          # fourteen pairs of the second block
    got, _, _ = RPush([s1(30, 40, wrong)]).check(emu)
    assert got[0][1] == dict(status=1, pairs=len(wrong), min_margin=got[0][1]["min_margin"], blocks=3)


def test_a_block_that_stays_bad_changes_nothing(emu):
    """Invalid pairs in two blocks; in the second the louder chip is the wrong one: status 2, no byte written, the record an abort."""
    a0, a1 = pair_chips(8 * 3 + 2)[0], pair_chips(8 * 20 + 5)[1]
    t = s1(31, 40, [a0, a1])
    loud = 0.3 if t.vals[a1] & 1 else -0.3                                      # the wrong chip, received loudly
    p = RPush([t, s1(32, 40, [a0, a1])], soft={(0, a1): loud})
    got, counters, taken = p.check(emu)
    assert got[0][0] == "subject" and got[0][1]["status"] == 2 and got[0][1]["pairs"] == 2 and got[0][1]["blocks"] == 3
    assert got[1][1]["status"] == 1 and taken == 48 and counters[1] - counters[0] == 48


def test_a_tie_reads_zero(emu):
    """Both soft symbols of an invalid pair equal: the bit is 0 -- right for a pair that was sent as 10, wrong for one sent as 01."""
    air = air_a(33, 40)
    body = TR.body("S1", air)
    zero = next(i for i in range(100, 300) if body[2 * i] == 1)                 # pair i was sent as 10: bit 0
    one = next(i for i in range(100, 300) if body[2 * i] == 0)
    tg = [Telegram("S1", air, flips=[pair_chips(zero)[0]]), Telegram("S1", air, flips=[pair_chips(one)[0]])]
    soft = {(0, pair_chips(zero)[0]): 0.125, (0, pair_chips(zero)[1]): 0.125, (1, pair_chips(one)[0]): -0.125, (1, pair_chips(one)[1]): -0.125}
    got, _, _ = RPush(tg, soft=soft).check(emu)
    assert got[0][1] == dict(status=1, pairs=1, min_margin=0, blocks=3)
    assert got[1][1] == dict(status=2, pairs=1, min_margin=0, blocks=3)


@pytest.mark.parametrize("lfield", [9, 25, 26, 255])
def test_lengths(emu, lfield):
    """L-field 9: L = 12, a single block, the smallest subject.  25 and 26: L = 30 and 33, a full second block and a last block of three
    bytes (frame A has no shorter last block: a block holds at least one byte and its CRC).  255: L = 290, 17 blocks, 4641 chips, 73
    trips of the wave."""
    L = TR.frame_a_length(lfield)
    wrong = sorted({pair_chips(8)[1], pair_chips(4 * L)[0], pair_chips(8 * L - 2)[1], pair_chips(8 * L - 1)[0]})
    got, _, _ = RPush([s1(40 + lfield, lfield, wrong)]).check(emu)
    kind, rec, b, a = got[0]
    assert kind == "subject" and rec == dict(status=1, pairs=len(wrong), min_margin=rec["min_margin"], blocks=RF.n_blocks(L)) and b["L"] == L
    assert RF.n_blocks(L) == {9: 1, 25: 2, 26: 3, 255: 17}[lfield]


def test_several_records_per_wave(emu):
    """One block of four waves walks fourteen records: every wave's scratch is used again, a long telegram's bits under a short one's."""
    lf = [255, 9, 40, 26, 9, 40, 25, 9, 40, 255, 9, 26, 40, 9]
    tg = []
    for k, f in enumerate(lf):
        L = TR.frame_a_length(f)
        tg.append(s1(60 + k, f, [pair_chips(8 + (5 * k) % (8 * L - 8))[k & 1]] if k % 5 != 4 else []))
    p = RPush(tg)
    got, counters, taken = p.check(emu, max_blocks=1)
    assert [got[k][1]["status"] for k in range(len(lf))] == [0 if k % 5 == 4 else 1 for k in range(len(lf))]
    assert all(got[k][2]["status"] == (DONE if k % 5 == 4 else ABORT) for k in range(len(lf)))
    assert counters[1] - counters[0] == taken
    for blocks in (2, 3):                                    # the same records whatever the grid
        again, _, _ = p.check(emu, max_blocks=blocks)
        assert [again[k][1] for k in range(len(lf))] == [got[k][1] for k in range(len(lf))]


def test_non_subjects_of_every_kind(emu):
    L = TR.frame_a_length(40)
    n = 1 + 16 * L
    c = pair_chips(100)[0]
    both = list(pair_chips(100))
    tg = [s1(80, 40),                                                       # 0: complete and clean
          s1(81, 40, both),                                                 # 1: both chips of a pair wrong: complete, a bad CRC -- CRC repair's subject
          s1(82, 40, [c], algo=0),                                          # 2: the run-length framer's
          Telegram("T1", air_a(83, 40), flips=[3]),                         # 3: the other chain's decoder gave up
          s1(84, 40, [pair_chips(3)[0]]),                                   # 4: an invalid pair inside the L-field: no length
          s1(85, 5, [pair_chips(20)[0]]),                                   # 5: L = 8 < 12
          s1(86, 40, [c]),                                                  # 6: the RSSI gate before the first invalid pair: consumed is the gate's
          s1(87, 40, [c]),                                                  # 7: a Manchester abort, the gate at chip n - 2 behind it
          s1(88, 40, [c]),                                                  # 8: the same at chip n - 1, the completing chip: exempt
          s1(89, 40, [c]),                                                  # 9: a Manchester abort, a framer reset on a later chip
          s1(90, 40, [c]),                                                  # 10: ... on the last chip
          s1(91, 40, [c])]                                                  # 11: the gate at chip 1 ... not below it: RSSI 5 passes
    tg[9].vals[c + 40] |= 4
    tg[10].vals[n - 1] |= 4
    rssi = {(6, c - 10): 4, (7, n - 2): 4, (8, n - 1): 0, (11, 1): 5, (11, n - 2): 5}
    got, _, _ = RPush(tg, rssi=rssi).check(emu)
    assert [got[k][2]["status"] for k in (0, 1)] == [DONE, DONE] and not got[1][2]["flags"] & PKTF_CRC
    assert all(got[k][2]["status"] == ABORT for k in range(2, 12))
    assert got[4][2]["L"] == 0 and got[5][2]["L"] == 8 and got[6][2]["consumed"] == c - 10 + 1
    assert [got[k][0] for k in range(12)] == ["no"] * 7 + ["gated", "subject", "gated", "gated", "subject"]
    assert [got[k][1]["status"] for k in range(12)] == [0] * 8 + [1, 0, 0, 1]
    assert got[8][3]["rssi_now"] == 0 and got[11][3]["pkt_rssi"] == 5


def test_an_arena_without_room(emu):
    """Three subjects of 47 bytes and an arena of 40, then of 100: storage first, as burst_item -- the telegram that finds no room is asked
    for once (the counter moves), a full arena is not asked again, and neither gives a line."""
    tg = [s1(95 + k, 40, [pair_chips(50 + k)[0]]) for k in range(3)]
    p = RPush(tg)
    got, counters, taken = p.check(emu, bytes_cap=40, max_blocks=1)
    assert [got[k][1]["status"] for k in range(3)] == [3, 3, 3] and taken == 0 and (counters[0], counters[1]) == (0, 48)
    got, counters, taken = p.check(emu, bytes_cap=100, max_blocks=1)
    assert sorted(got[k][1]["status"] for k in range(3)) == [1, 1, 3] and taken == 96 and (counters[0], counters[1]) == (0, 144)
    assert all(got[k][2]["status"] == got[k][3]["status"] == ABORT for k in range(3))
