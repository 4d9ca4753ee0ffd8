"""Channel power (cfg.line_power): the device source of the band form of the survey kernel (rtl-wmbus_amd/csrc/wm_k0_spectrum.h:
k0_spectrum_block<FMT, DC, AGE, true>) and of k0_channel_power (wm_k0_power.h) on the coroutine block emulator against the restatement
tests/power_ref.py, exact.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import afc_age_ref as AG
import format_ref as FR
import power_ref as PW
import spectrum_ref as PR
from test_formats_emulated import FMT_IDS, FORMATS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libpower_emu.so")
SRC = os.path.join(HERE, "emu", "power_emu.cpp")
FS = 1600000
RUN = 4                                             # level blocks per wave as the host chooses them for a push below 16384 level blocks (spec_launch)
RUN_LONG = 16                                       # ... and from there on


def load_emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h")] + [os.path.join(CSRC, h) for h in ("wm_k0_resample.h", "wm_k0_spectrum.h", "wm_k0_afc.h", "wm_k0_power.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    L.wm_emu_pow_new.restype = vp
    L.wm_emu_pow_new.argtypes = [ctypes.c_uint, vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint64]
    L.wm_emu_pow_free.argtypes = [vp]
    L.wm_emu_pow_push.restype = ctypes.c_long
    L.wm_emu_pow_push.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.wm_emu_pow_read.restype = ctypes.c_long
    L.wm_emu_pow_read.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_uint64)]
    L.wm_emu_pow_channel.restype = None
    L.wm_emu_pow_channel.argtypes = [vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, vp, vp, vp, vp]
    L.wm_emu_pow_window.restype = None
    L.wm_emu_pow_window.argtypes = [ctypes.c_uint, ctypes.c_int64, vp]
    return L


@pytest.fixture(scope="module")
def emu():
    return load_emu()


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.line_power: on a library without the field no test of this file says anything, so none passes."""
    assert "line_power" in [f[0] for f in wm.Cfg._fields_] and "wmbus_read_waterfall" in wm.EXPORTS


def run_emulated(emu, wm, raw, fmt, R, cuts, run, age=0):
    """(rows uint32 [blocks, 32] of the whole stream, (sum, peak, blocks) behind the last push)."""
    table = wm.shift_design(FS, 0)[1]
    h = emu.wm_emu_pow_new(fmt, table.ctypes.data, R, run, age, 0)
    try:
        off, rows = 0, []
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            n_blk = n // FR.BPS[fmt] // PR.N
            out = np.zeros((n_blk, 32), np.uint32)
            assert emu.wm_emu_pow_push(h, part.ctypes.data, part.size, out.ctypes.data) == n_blk
            rows.append(out)
        assert off == raw.size
        total, peak, blocks = np.zeros(PR.N, np.uint64), np.zeros(PR.N, np.uint32), ctypes.c_uint64()
        emu.wm_emu_pow_read(h, total.ctypes.data, peak.ctypes.data, ctypes.byref(blocks))
        return np.concatenate(rows), (total, peak, int(blocks.value))
    finally:
        emu.wm_emu_pow_free(h)


def tone_on_a_bin_centre(fmt, n_blk, b=37):
    """A full-scale complex tone on the centre of bin 256 + b: the largest band there is from a tone -- the bin and its two Hann
    neighbours, a quarter each, share band (256 + b) // 16.  (The clamp of a band at 2^32 - 1 is a guard no input reaches: by Parseval
    the pw of ALL 512 bins of a level block add up to 512 x sum |y|^2 >> 16 <= 512 x 192 x 2^31 >> 16 = 0.75 x 2^32, 192 being the
    sum of the squared Hann window.  k0_channel_power's clamp is reached with synthetic rows below.)"""
    n = n_blk * PR.N
    w = 2.0 * np.pi * b * np.arange(n) / PR.N
    tone = np.stack([np.cos(w), np.sin(w)], axis=1).reshape(-1)
    if fmt == FR.CU8:
        v = np.clip(np.rint(127.5 + 127.5 * tone), 0, 255)
    elif fmt == FR.CS8:
        v = np.clip(np.rint(-0.5 + 127.5 * tone), -128, 127)
    elif fmt == FR.CS16:
        v = np.clip(np.rint(32767.5 * tone - 0.5), -32768, 32767)
    else:
        v = tone.astype(np.float32)
    return FR.raw_bytes(v, fmt)


def level_blocks(fmt, n_blk, kind, seed=0):
    nbytes = n_blk * PR.N * FR.BPS[fmt]
    if kind == "random":
        return np.random.default_rng(0xB0 + fmt + seed).integers(0, 256, nbytes, dtype=np.uint8)
    if kind == "silence":
        return np.full(nbytes, {FR.CU8: 128, FR.CS8: 0, FR.CS16: 0, FR.CF32: 0}[fmt], np.uint8)
    return tone_on_a_bin_centre(fmt, n_blk)


def per_4096(fmt):
    return 4096 // FR.BPS[fmt] // PR.N                            # level blocks of one 4096-byte unit: 4 / 4 / 2 / 1


@pytest.mark.parametrize("R", [0, 6], ids=["R0", "R6"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_band_rows_of_the_device_source_match_the_restatement(emu, wm, fmt, R):
    """Four formats, with and without the DC table; pushes of 1, 3, run, run + 1 and 4 run + 1 level blocks where the format's 4096-byte
    unit allows (a push is whole units: the 8-bit formats take the next multiple of 4 level blocks), one after the other on ONE stream
    so that the blocker's state and the accumulators carry; random bytes (NaN and infinities among the cf32 ones), silence and the
    full-scale tone on a bin centre (the largest band a tone gives).  The accumulators beside the rows are still the survey's."""
    u = per_4096(fmt)
    pushes = [-(-n // u) * u for n in (1, 3, RUN, RUN + 1, 4 * RUN + 1)]
    cuts = [n * PR.N * FR.BPS[fmt] for n in pushes]
    for kind in ("random", "silence", "tone"):
        raw = level_blocks(fmt, sum(pushes), kind)
        want = PW.band_rows(raw, fmt, R)
        rows, acc = run_emulated(emu, wm, raw, fmt, R, cuts, RUN)
        assert rows.shape == want.shape and np.array_equal(rows, want), kind
        survey = PR.spectrum(raw, fmt, R)
        assert acc[2] == survey[2] and np.array_equal(acc[0], survey[0]) and np.array_equal(acc[1], survey[1]), kind
        rows16, _ = run_emulated(emu, wm, raw, fmt, R, [raw.size], RUN_LONG)        # one push, the long run: a wave's last run is partial
        assert np.array_equal(rows16, want), kind
        if kind == "silence" and fmt in (FR.CS16, FR.CF32):
            assert not want.any()
        if kind == "tone" and not R:
            b = (256 + 37) // 16
            assert int(want[0].argmax()) == b and int(want.max()) < 3 << 30
            if fmt in (FR.CS16, FR.CF32):                         # (an 8-bit sample is widened x 64 only: 2^-4 of full scale in power)
                assert int(want[:, b].min()) > 1 << 30
            assert int(np.delete(want, b, axis=1).max()) < int(want[:, b].min()) >> 12


@pytest.mark.parametrize("fmt", [FR.CU8, FR.CS16, FR.CF32], ids=["cu8", "cs16", "cf32"])
def test_the_ageing_form_writes_every_row_and_keeps_its_view(emu, wm, fmt):
    """A = 2 and pushes of 32 level blocks: all but the last 5 ... 8 level blocks of such a push lie in epochs the view no longer holds --
    the plain AGE form leaves them untransformed -- and every one of the 32 rows is present all the same; the view behind every push is
    still tests/afc_age_ref.py's.  A third push of 4 level blocks ends inside an epoch."""
    A, u = 2, per_4096(fmt)
    pushes = [32, 32, -(-3 // u) * u, 32]
    cuts = [n * PR.N * FR.BPS[fmt] for n in pushes]
    raw = level_blocks(fmt, sum(pushes), "random", seed=9)
    want = PW.band_rows(raw, fmt)
    pw = AG.stream_power(raw, fmt)
    table = wm.shift_design(FS, 0)[1]
    h = emu.wm_emu_pow_new(fmt, table.ctypes.data, 0, RUN, A, 0)
    try:
        off = K = 0
        for n_blk, nbytes in zip(pushes, cuts):
            part = np.ascontiguousarray(raw[off:off + nbytes]); off += nbytes
            out = np.zeros((n_blk, 32), np.uint32)
            assert emu.wm_emu_pow_push(h, part.ctypes.data, part.size, out.ctypes.data) == n_blk
            assert np.array_equal(out, want[K:K + n_blk]), K
            K += n_blk
            total, peak, blocks = np.zeros(PR.N, np.uint64), np.zeros(PR.N, np.uint32), ctypes.c_uint64()
            emu.wm_emu_pow_read(h, total.ctypes.data, peak.ctypes.data, ctypes.byref(blocks))
            v = AG.view(pw, K - 1, A)
            assert int(blocks.value) == v[2] and np.array_equal(total, v[0]) and np.array_equal(peak, v[1]), K
            assert v[2] < n_blk or n_blk < 32
    finally:
        emu.wm_emu_pow_free(h)


def channel_emulated(emu, rows, n_ch, fin, centre_hz, chain_hz, held=None):
    """P uint32 [2 S, n_blk] of k0_channel_power_block; rows [n_cap, n_blk, 32]."""
    rows = np.ascontiguousarray(rows, np.uint32)
    n_cap, n_blk = rows.shape[0], rows.shape[1]
    S = n_cap * n_ch
    P = np.zeros((2 * S, n_blk), np.uint32)
    c = np.ascontiguousarray(list(centre_hz) + [0] * (8 - len(centre_hz)), np.int32)
    ch = np.ascontiguousarray(chain_hz, np.int32)
    hd = None if held is None else np.ascontiguousarray(held, np.int32)
    emu.wm_emu_pow_channel(rows.ctypes.data, n_cap, n_ch, n_blk, fin, c.ctypes.data, ch.ctypes.data, None if hd is None else hd.ctypes.data, P.ctypes.data)
    return P


@pytest.mark.parametrize("fin", [800000, 1600000, 2400000, 4000000, 10000000])
def test_channel_power_of_the_device_source_matches_the_restatement(emu, fin):
    """Random band rows (a fifth of them at or near the clamp, so that sums of nb bands clamp too) of two captures; a fixed shift, a
    channel list, -s, and AFC states; 1, 7, 8, 9 and 21 level blocks (a block of threads takes 8)."""
    rng = np.random.default_rng(fin)
    for n_blk in (1, 7, 8, 9, 21):
        rows = rng.integers(0, 1 << 32, (2, n_blk, 32), dtype=np.uint64).astype(np.uint32)
        rows[rng.random(rows.shape) < 0.2] = PW.U32
        rows[rng.random(rows.shape) < 0.3] >>= 12
        cases = [(1, [-123456], (0, 0), None), (1, [0], (PW.SIM_HZ, -PW.SIM_HZ), None),
                 (3, [fin // 2, -(fin // 2), 31250], (0, 0), None), (3, [250000, -325000, 0], (PW.SIM_HZ, -PW.SIM_HZ), None),
                 (1, [0], (0, 0), [40000, -fin // 4]), (2, [0, 0], (PW.SIM_HZ, -PW.SIM_HZ), [1, -1, fin // 2, -(fin // 2)])]
        saw_clamp = False
        for n_ch, centre, chain, held in cases:
            P = channel_emulated(emu, rows, n_ch, fin, centre, chain, held)
            S = 2 * n_ch
            for chn in range(2):
                for v in range(S):
                    f = (held[v] if held is not None else centre[v % n_ch]) + chain[chn]
                    want = PW.channel_power(rows[v // n_ch], fin, f)
                    assert np.array_equal(P[chn * S + v], want), (n_blk, n_ch, chn, v)
                    saw_clamp |= bool((want == PW.U32).any())
        assert saw_clamp or n_blk == 1


def test_chain_rows_differ_by_the_simultaneous_shift():
    """With -s the two chains of a stream look at windows 650 kHz apart: T1/C1 above the centre, S1 below."""
    fin = 2400000
    assert PW.chain_hz(0, True) == 325000 and PW.chain_hz(1, True) == -325000 and PW.chain_hz(0, False) == 0
    assert PW.centre(fin, 325000)[0] - PW.centre(fin, -325000)[0] in (138, 139)       # 650 kHz / 4687.5 Hz per bin = 138.7
