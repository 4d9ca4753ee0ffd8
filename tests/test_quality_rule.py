"""Line quality (cfg.line_quality): the rule of include/wmbus_hip.h, LINE QUALITY, as tests/quality_ref.py restates it -- closed forms
of the timing figures, the corners of the eye figures, the invalid records, the records of the bundled capture -- and the ABI of the
feature.  No GPU needed.  Fails on a tree without the feature."""
import ctypes
import json
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import quality_ref as QR
from conftest import ROOT

# the issue's table: the two time2 telegrams of the bundled 1.6 MS/s capture
TABLE = [dict(n=577, chip_rate_chz=9980014, jitter_ns=1367, hi_hz=41642, lo_hz=-68343, spread_hz=7986, eye_hz=32214),
         dict(n=1405, chip_rate_chz=9976530, jitter_ns=775, hi_hz=35858, lo_hz=-61937, spread_hz=6924, eye_hz=-9951)]


def soft(pos, v, amp=0.125, row=None):
    """A soft-symbol row with +amp under the chips of value 1 and -amp under the others."""
    pos = np.asarray(pos, np.int64)
    row = np.zeros(int(pos[-1]) + 1, np.float32) if row is None else row
    row[pos] = np.where(np.asarray(v) & 1, amp, -amp).astype(np.float32)
    return row


def alternating(n):
    return np.arange(n) & 1


def least_squares(pos):
    """(slope in samples per chip, mean absolute residual in samples) of the least-squares line through (j, pos[j]), in fractions."""
    n = len(pos)
    jm, pm = Fraction(n - 1, 2), Fraction(sum(int(x) for x in pos), n)
    b = sum((j - jm) * (int(p) - pm) for j, p in enumerate(pos)) / sum((j - jm) ** 2 for j in range(n))
    a = pm - b * jm
    return b, sum(abs(int(p) - a - b * j) for j, p in enumerate(pos)) / n


# ---- timing -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,rate", [(8, 10_000_000), (9, 8_888_889)])
def test_an_exact_grid(step, rate):
    n = 145
    pos = 1000 + step * np.arange(n)
    rec = QR.quality(pos, alternating(n), soft(pos, alternating(n)))
    assert (rec["n"], rec["chip_rate_chz"], rec["jitter_ns"]) == (n, rate, 0)


def test_s1_nominal_clock_off_the_sample_grid():
    """pos[j] = floor(3125 j / 128): 32 768 chip/s at 800 kHz.  The rate within one unit of the exact least squares; the jitter is that
    of whole-sample positions: a few hundred ns, not 0."""
    n = 1 + 16 * 40
    pos = 3125 * np.arange(n) // 128
    rec = QR.quality(pos, alternating(n), soft(pos, alternating(n)))
    b, resid = least_squares(pos)
    assert abs(rec["chip_rate_chz"] - Fraction(80_000_000) / b) <= 1
    # every position is up to one sample early: a perturbation within a band of 1 sample moves a least-squares slope by at most
    # 0.5 sum |j - mean| / sum (j - mean)^2 < 1.5 / n samples per chip
    assert abs(rec["chip_rate_chz"] - 3_276_800) <= 3_276_800 * Fraction(3, 2 * n) * Fraction(128, 3125) + 1
    assert abs(rec["jitter_ns"] - 1250 * resid) <= 1250 * Fraction(n + 1, 1 << 17) + 1
    assert 100 < rec["jitter_ns"] < 625


def test_one_slip_in_the_middle():
    """An exact grid of 8 with one slip of + 8 samples half way: against a least-squares fit in fractions.  B is the slope to 2^-17
    sample per chip and A the intercept to 2^-17 sample, so a residual is off by at most (n + 1) 2^-17 samples; one unit for the floor."""
    n = 145
    pos = 8 * np.arange(n) + np.where(np.arange(n) >= n // 2, 8, 0)
    rec = QR.quality(pos, alternating(n), soft(pos, alternating(n)))
    b, resid = least_squares(pos)
    assert abs(rec["chip_rate_chz"] - Fraction(80_000_000) / b) <= 1
    assert abs(rec["jitter_ns"] - 1250 * resid) <= 1250 * Fraction(n + 1, 1 << 17) + 1
    assert rec["jitter_ns"] > 1500 and rec["chip_rate_chz"] < 10_000_000


# ---- eye ----------------------------------------------------------------------------------------------------------------------------
def test_eye_of_clean_symbols():
    n = 145
    pos, v = 8 * np.arange(n), alternating(n)
    rec = QR.quality(pos, v, soft(pos, v))
    q = 1 << 17                                                     # 0.125 x 2^20
    assert (rec["hi_hz"], rec["lo_hz"], rec["spread_hz"], rec["eye_hz"]) == (QR.hz(q, 1), QR.hz(-q, 1), 0, QR.hz(q, 1)) == (50000, -50000, 0, 50000)


def test_inverted_polarity():
    """sigma = -1: ones below zeros.  The eye is as open as it is the other way round."""
    n = 145
    pos, v = 8 * np.arange(n), alternating(n)
    rec = QR.quality(pos, v, soft(pos, v, amp=-0.125))
    assert (rec["hi_hz"], rec["lo_hz"], rec["eye_hz"], rec["spread_hz"]) == (-50000, 50000, 50000, 0)


def test_a_chip_on_the_wrong_side():
    n = 145
    pos, v = 8 * np.arange(n), alternating(n)
    row = soft(pos, v)
    row[pos[71]] = -0.03125                                          # a one that reads as a weak zero
    rec = QR.quality(pos, v, row)
    m1 = (2 * (71 * (1 << 17) - (1 << 15)) + 72) // (2 * 72)
    mid = (m1 - (1 << 17)) // 2
    assert rec["eye_hz"] == QR.hz(-(1 << 15) - mid, 1) < 0 and rec["hi_hz"] == QR.hz(m1, 1) and rec["spread_hz"] > 0


def test_nan_soft_symbol_counts_as_zero():
    n = 145
    pos, v = 8 * np.arange(n), alternating(n)
    row, zero = soft(pos, v), soft(pos, v)
    row[pos[71]], zero[pos[71]] = np.nan, 0.0
    rec = QR.quality(pos, v, row)
    assert rec == QR.quality(pos, v, zero) and rec["n"] == n and 0 < rec["eye_hz"] < 1000


def test_clamped_symbols_need_64_bit_sums():
    """2100 ones at the clamp: S1 = 2100 x 2^20 > 2^31."""
    n = 4200
    pos, v = 8 * np.arange(n), alternating(n)
    rec = QR.quality(pos, v, soft(pos, v, amp=3.0))
    assert (rec["hi_hz"], rec["lo_hz"], rec["spread_hz"], rec["eye_hz"]) == (400000, -400000, 0, 400000)
    assert rec["chip_rate_chz"] == 10_000_000 and rec["jitter_ns"] == 0


# ---- invalid ------------------------------------------------------------------------------------------------------------------------
def test_invalid_records():
    n = 145
    pos, v = 8 * np.arange(n), alternating(n)
    row = soft(pos, v)
    assert QR.quality(pos, np.ones(n, np.int64), row) == QR.ZERO and QR.quality(pos, np.zeros(n, np.int64), row) == QR.ZERO
    assert QR.quality(pos[:1], v[:1], row) == QR.ZERO
    assert QR.quality(pos[:2], v[:2], row)["n"] == 2
    wide = np.array([0, (1 << 17) - 1]); assert QR.quality(wide, [0, 1], soft(wide, [0, 1]))["n"] == 2
    wide = np.array([0, 1 << 17]); assert QR.quality(wide, [0, 1], soft(wide, [0, 1])) == QR.ZERO
    assert QR.quality([5, 5], [0, 1], row) == QR.ZERO               # num = 0


# ---- the captures -------------------------------------------------------------------------------------------------------------------
def test_golden_is_a_fresh_run_and_the_bundled_capture_reads_as_the_table(oracle, samples):
    with open(QR.GOLDEN) as f:
        gold = json.load(f)
    cu8 = samples["samples2"][:samples["samples2"].size // 4096 * 4096]
    ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
    recs = QR.quality_capture(ref)
    assert gold["samples2"]["lines"] == ref["text"].splitlines(keepends=True) and gold["samples2"]["records"] == recs
    assert [recs[0], recs[2]] == TABLE and recs[1] == recs[3] == QR.ZERO
    # the cut is a parameter: the telegrams' chips lie in decimated samples 192 156 ... 196 772 and 364 951 ... 376 208, so pushes of
    # 2^17 keep both whole, pushes of 2^16 cut the first (196 608 = 3 x 2^16) and pushes of 2^12 both
    assert QR.quality_capture(ref, push_m=1 << 17) == recs
    assert QR.quality_capture(ref, push_m=1 << 16) == [QR.ZERO, QR.ZERO, recs[2], QR.ZERO]
    assert QR.quality_capture(ref, push_m=1 << 12) == [QR.ZERO] * 4
    for name, (mode, sigma) in QR.RR.SYNTHETIC.items():
        cu8, _ = QR.RR.synthetic(mode, sigma)
        ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
        tg = sorted(QR.RR.telegrams(ref, 0) + QR.RR.telegrams(ref, 1), key=lambda t: (t["sample"], t["chain"]))[:6]
        got = [QR.quality_telegram(t, ref["dphi_fir"][t["chain"]]) for t in tg]
        assert got == gold["synthetic"][name]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_abi_has_the_quality(wm):
    """The field sits directly in front of tolerance_mode: the last seam no earlier test pinned."""
    names = [f[0] for f in wm.Cfg._fields_]
    i = names.index("line_quality")
    assert names[i - 1] == "input_windows" and names[i + 1:i + 3] == ["tolerance_mode", "crc_repair"]
    with open(os.path.join(ROOT, "include", "wmbus_hip.h")) as f:
        assert "directly in front of tolerance_mode" in f.read()
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(wmbus_cfg), '
                           'offsetof(wmbus_cfg, line_quality), offsetof(wmbus_cfg, tolerance_mode), sizeof(wmbus_quality), offsetof(wmbus_quality, eye_hz), '
                           'offsetof(wmbus_quality, hi_hz));return 0;}\n')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(wm.Cfg), wm.Cfg.line_quality.offset, wm.Cfg.tolerance_mode.offset, ctypes.sizeof(wm.Quality), wm.Quality.eye_hz.offset,
                   wm.Quality.hi_hz.offset]
    assert ctypes.sizeof(wm.Quality) == 32 and wm.Quality.eye_hz.offset == 24 and wm.Cfg.tolerance_mode.offset == wm.Cfg.line_quality.offset + 4
    c = wm.Cfg()
    c.line_quality = 7
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.line_quality == 0
    for name in ("wmbus_line_quality", "wmbus_batch_line_quality"):
        assert name in wm.EXPORTS and hasattr(wm.lib(), name)
    assert hasattr(wm.Receiver, "line_quality")
    p = ctypes.POINTER(wm.Quality)()
    assert wm.lib().wmbus_line_quality(None, ctypes.byref(p)) == 0 and not p
    assert wm.lib().wmbus_batch_line_quality(None, 0, ctypes.byref(p)) == 0 and not p


def test_the_field_is_validated_before_a_device_is_asked_for(wm):
    """WMBUS_EINVAL (-1) with a message, on any machine: above 1; together with bursts_to_host."""
    with pytest.raises(wm.WmbusError, match=r"\(-1\): line_quality must be 0 or 1, got 2"):
        wm.Receiver(n_streams=1, line_quality=2)
    with pytest.raises(wm.WmbusError, match=r"\(-1\): line_quality .* bursts_to_host .* nothing it could measure"):
        wm.Receiver(n_streams=1, line_quality=1, bursts_to_host=True)
    with pytest.raises(wm.WmbusError, match=r"line_quality must be 0 or 1, got 3"):
        wm.Batch(n_streams=64, line_quality=3)


def test_cli_knows_the_switch(wm):
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert p.stdout.count("\t-q append ;<chip rate, chips/s, two decimals>;<jitter ns>;<eye Hz> to every line") == 1
