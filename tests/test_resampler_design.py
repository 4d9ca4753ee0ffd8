"""wmbus_resampler_design (host only): geometry, exact phase sums, symmetry, agreement with an independent scipy design, and the
frequency response of the int16 prototype.  No GPU needed.

The two response limits were set from a scipy prototype of exactly this design before the library's existed: pass-band ripple
0.002 ... 0.208 dB (worst: 3 MS/s) and stop band -68.0 ... -81.4 dB after Q14 rounding (worst: 10 MS/s; the float design has
-80 ... -86 dB).  0.25 dB and -65 dB hold every rate with 3 dB to spare on the worst, far below an 8-bit input's quantisation noise."""
import ctypes
import math

import numpy as np
import pytest

# (input rate, decimation) -> L, M
RATES = [(2048000, 2, 25, 32), (2000000, 2, 4, 5), (2400000, 2, 2, 3), (2560000, 2, 5, 8), (3000000, 2, 8, 15),
         (1000000, 1, 4, 5), (10000000, 2, 4, 25)]
IDS = [f"{r[0]}-d{r[1]}" for r in RATES]


def rounded_scipy_design(fin, fout, L, T):
    """The same design, independently: firwin prototype, each phase scaled to sum 1, times 16384, rounded (no adjustment)."""
    from scipy.signal import firwin
    h = firwin(L * T, 0.45 * min(fin, fout), window=("kaiser", 8), fs=L * fin)
    ph = h.reshape(T, L).T                                  # phase p: prototype taps p, p + L, ...
    return np.rint(ph / ph.sum(axis=1, keepdims=True) * 16384).astype(np.int64)


@pytest.mark.parametrize("fin,d,L,M", RATES, ids=IDS)
def test_geometry_and_phase_sums(wm, fin, d, L, M):
    gL, gM, T, taps = wm.resampler_design(fin, 800000 * d)
    assert (gL, gM) == (L, M)
    assert T == min(512, 16 * max(1, math.ceil(M / L)))
    assert taps.shape == (L, T) and taps.dtype == np.int16
    assert np.all(taps.astype(np.int64).sum(axis=1) == 16384)
    # the accumulator bound: 255 * sum|taps| < 2^23
    assert 255 * np.abs(taps.astype(np.int64)).sum(axis=1).max() < 2 ** 23


@pytest.mark.parametrize("fin,d,L,M", RATES, ids=IDS)
def test_taps_agree_with_an_independent_scipy_design(wm, fin, d, L, M):
    _, _, T, taps = wm.resampler_design(fin, 800000 * d)
    ref = rounded_scipy_design(fin, 800000 * d, L, T)
    diff = taps.astype(np.int64) - ref
    for p in range(L):
        big = int(np.argmax(np.abs(taps[p].astype(np.int64))))        # where the library put the phase's adjustment
        others = np.delete(diff[p], big)
        assert np.abs(others).max() <= 1, (p, others)
        # the adjusted tap: 1 LSB, plus what the reference's rounded phase misses of 16384, plus the other taps' disagreements
        assert abs(diff[p, big]) <= 1 + abs(16384 - ref[p].sum()) + np.abs(others).sum(), (p, diff[p, big])


@pytest.mark.parametrize("fin,d,L,M", RATES, ids=IDS)
def test_prototype_is_symmetric_up_to_the_adjustment(wm, fin, d, L, M):
    _, _, T, taps = wm.resampler_design(fin, 800000 * d)
    ref = rounded_scipy_design(fin, 800000 * d, L, T)
    # per phase, the most an adjusted tap can be away from its rounded value
    adj = np.abs(16384 - ref.sum(axis=1)) + np.abs(taps.astype(np.int64) - ref).sum(axis=1)
    h = taps.astype(np.int64).T.reshape(-1)                  # h[p + L k]
    N = h.size
    phase = np.arange(N) % L
    allowed = adj[phase] + adj[phase[::-1]]
    assert np.all(np.abs(h - h[::-1]) <= allowed)
    # and apart from the (at most 2 L) adjusted taps it is exactly symmetric
    assert np.count_nonzero(h != h[::-1]) <= 2 * L


@pytest.mark.parametrize("fin,d,L,M", RATES, ids=IDS)
def test_frequency_response_of_the_int16_prototype(wm, fin, d, L, M):
    fout = 800000 * d
    _, _, T, taps = wm.resampler_design(fin, fout)
    h = taps.astype(np.float64).T.reshape(-1) / (16384.0 * L)      # unity gain at DC at the rate L * fin
    NF = 1 << 20
    H = np.abs(np.fft.rfft(h, NF))
    f = np.arange(H.size) * (L * fin / NF)
    lo = min(fin, fout)
    pb = 20 * np.log10(H[f <= 0.35 * lo])
    sb = 20 * np.log10(np.maximum(H[f >= 0.6 * lo], 1e-12))
    ripple, stop = float(np.abs(pb).max()), float(sb.max())
    print(f"{fin} -> {fout}: pass-band ripple {ripple:.4f} dB, stop band {stop:.2f} dB")
    assert ripple <= 0.25
    assert stop <= -65.0


@pytest.mark.parametrize("fin,fout", [(700000, 1600000), (2047999, 1600000), (1600001, 1600000), (40000000, 800000), (2048000, 1000000),
                                      (2048000, 0)])
def test_unsupported_ratios_are_einval(wm, fin, fout):
    u = ctypes.c_uint
    L_, M_, T_ = u(), u(), u()
    assert wm.lib().wmbus_resampler_design(fin, fout, ctypes.byref(L_), ctypes.byref(M_), ctypes.byref(T_), None, 0) == -1
    with pytest.raises(wm.WmbusError):
        wm.resampler_design(fin, fout)


def test_tap_buffer_too_small_is_einval(wm):
    u = ctypes.c_uint
    L_, M_, T_ = u(), u(), u()
    buf = np.zeros(16, np.int16)
    assert wm.lib().wmbus_resampler_design(2048000, 1600000, ctypes.byref(L_), ctypes.byref(M_), ctypes.byref(T_), buf.ctypes.data, buf.size) == -1
