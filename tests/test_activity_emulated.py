"""Channel activity (cfg.channel_activity): the device source of k0_activity (rtl-wmbus_amd/csrc/wm_k0_activity.h: k0_activity_wave) on the
coroutine block emulator against the restatement tests/activity_ref.py, exact, with the stream cut into pushes so that every carry offset
occurs.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import activity_ref as AR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libactivity_emu.so")
SRC = os.path.join(HERE, "emu", "activity_emu.cpp")
CASES = AR.cases()


def load_emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k0_resample.h", "wm_k0_spectrum.h", "wm_k0_afc.h", "wm_k0_power.h", "wm_k0_activity.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    L.wm_emu_act_new.restype = vp
    L.wm_emu_act_new.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
    L.wm_emu_act_free.argtypes = [vp]
    L.wm_emu_act_push.restype = ctypes.c_long
    L.wm_emu_act_push.argtypes = [vp, vp, ctypes.c_uint, vp, ctypes.c_size_t]
    L.wm_emu_act_state.restype = None
    L.wm_emu_act_state.argtypes = [vp, ctypes.c_uint, vp]
    L.wm_emu_act_epochs.restype = ctypes.c_uint
    L.wm_emu_act_epochs.argtypes = [ctypes.c_uint]
    L.wm_emu_act_row_cap.restype = ctypes.c_uint
    L.wm_emu_act_row_cap.argtypes = [ctypes.c_uint]
    return L


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.channel_activity: on a library without the field no test of this file says anything, so none passes."""
    assert "channel_activity" in [f[0] for f in wm.Cfg._fields_] and "wmbus_activity" in wm.EXPORTS


def run_emulated(emu, rows_p, fin, T, pushes, count0=0):
    """rows_p: [rows][n] timelines of equal length; pushes: [(start, stop)].  Returns ([records per row, concatenated over the pushes],
    carry offsets seen in row 0)."""
    P = np.ascontiguousarray(rows_p, np.uint32)
    rows = P.shape[0]
    h = emu.wm_emu_act_new(rows, fin, T, count0)
    got, offsets = [[] for _ in range(rows)], set()
    st = np.zeros(3, np.uint64)
    try:
        for a, b in pushes:
            emu.wm_emu_act_state(h, 0, st.ctypes.data)
            assert int(st[0]) == a % 64 and int(st[1]) == a // 64                # the state has advanced once per push
            offsets.add(int(st[0]))
            part = np.ascontiguousarray(P[:, a:b])
            cap = rows * emu.wm_emu_act_row_cap(b - a)
            out = np.zeros((cap, 5), np.uint64)
            n = emu.wm_emu_act_push(h, part.ctypes.data, b - a, out.ctypes.data, cap)
            assert 0 <= n <= cap
            last = (-1, -1)
            for first, blocks, mean, floor, row in out[:n].tolist():
                assert (row, first) > last                                       # rows ascending, first_block ascending
                last = (row, first)
                got[row].append(dict(first_block=first, blocks=blocks, mean=mean, floor=floor))
    finally:
        emu.wm_emu_act_free(h)
    return got, offsets


def three_rows(name):
    """The case's timeline in the middle row; another case's (cut or padded with its own first value) and a rolled copy beside it."""
    p, fin, T = CASES[name]
    other = CASES["random" if name != "random" else "lane_0_and_63"][0]
    other = np.resize(other, p.size)
    return [other, p, np.roll(p, 29)], fin, T


def test_the_emulator_shares_the_helpers(emu):
    for fin in (800000, 1600000, 2400000, 4000000, 12492800, 12595200, 12800000, 20000000):
        assert emu.wm_emu_act_epochs(fin) == AR.epochs_back(fin)
    assert [emu.wm_emu_act_row_cap(n) for n in (1, 64, 4096)] == [(1 + 63) // 3 + 2, (64 + 63) // 3 + 2, (4096 + 63) // 3 + 2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_kernel_is_the_restatement_whatever_the_cut(emu, name):
    """Three rows per launch (a row's state cannot leak), the stream cut into pushes of 1, 3, 64, 5 and 67 level blocks in turn, pushed
    whole, and in pushes of 1 and 2 level blocks, with which every carry offset 0 ... 63 occurs."""
    rows_p, fin, T = three_rows(name)
    want = [AR.rule(p, fin, T) for p in rows_p]
    n = rows_p[1].size
    got, offsets = run_emulated(emu, rows_p, fin, T, AR.cut(n))
    assert got == want
    whole, _ = run_emulated(emu, rows_p, fin, T, [(0, n)])
    assert whole == want
    # 1 + 3 + 64 + 5 + 67 = 140 = 12 mod 64: those pushes start at offsets 0, 1, 4 and 9 mod 4 only.  Pushes of 1 and 2 level blocks in
    # turn (3 per round, coprime to 64) start at every offset 0 ... 63 within 192 level blocks
    small, more = run_emulated(emu, rows_p, fin, T, AR.cut(n, (1, 2)))
    assert small == want
    assert n < 192 or more == set(range(64)), sorted(set(range(64)) - more)
    assert {0, 1, 4} <= offsets


def test_other_cuts_and_a_wrapping_ticket_counter(emu):
    """Pushes of 63, 65 and 128 level blocks, and tickets that wrap past 2^32 in mid-stream."""
    rows_p, fin, T = three_rows("random")
    want = [AR.rule(p, fin, T) for p in rows_p]
    n = rows_p[1].size
    for units in ((63,), (65,), (128, 1), (2, 190)):
        got, _ = run_emulated(emu, rows_p, fin, T, AR.cut(n, units), count0=2 ** 32 - 3)
        assert got == want, units


def test_a_run_per_three_blocks_fills_the_region_exactly(emu):
    """The worst case the arena is sized for: two active, one inactive, for ever."""
    n = 64 * 6
    p = np.full(n, 100, np.uint32)
    p[np.arange(n) % 3 != 2] = 5000                      # 43 of 64 blocks high: the quartile would be high -- a quiet first epoch keeps the floor low
    p[:64] = 100
    want = AR.rule(p, 1600000, 0)
    assert len(want) >= (n - 128) // 3
    for pushes in ([(0, n)], AR.cut(n), AR.cut(n, (64,))):
        got, _ = run_emulated(emu, [p, p], 1600000, 0, pushes)
        assert got == [want, want]
