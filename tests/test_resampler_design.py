"""wmbus_resampler_design (host only): geometry, exact phase sums, symmetry, agreement with an independent scipy design, and the
frequency response of the int16 prototype -- at seven everyday rates, and (second half of the file) over the whole design space
that tests/resample_ref.py enumerates: all 5750 (L, M) designs for geometry, sums, accumulator bounds, tile and LDS; the corners and
a seeded sample of them for the response.  No GPU needed.

The two response limits of the seven rates were set from a scipy prototype of exactly this design before the library's existed:
pass-band ripple 0.001 ... 0.207 dB (worst: 3 MS/s) and stop band -70.4 ... -82.1 dB after Q14 rounding (worst: 10 MS/s; the float
design has -80 ... -86 dB).  0.25 dB and -65 dB hold THESE SEVEN rates with 5 dB to spare on the worst, far below an 8-bit input's
quantisation noise.  They do not hold the whole space (ripple dB / stop band dB, worst per class of T, 78 designs: the corners and
the default sample):

    T            float64 design      the library's int16 taps
    16 .. 64     0.328 / -57.9       0.328 / -58.1      M / L whole or just below a whole number: ceil leaves T no slack, the
    80 .. 240    0.295 / -61.5       0.296 / -61.6      Kaiser transition from 0.45 does not reach the stop band by 0.6
    256 .. 512   0.286 / -62.7       0.280 / -57.9      Q14 rounding: the largest tap is below 500

test_response_against_the_float_design holds the int16 taps against the float design plus the predicted rounding floor.  It is the
test that found the earlier rule for the phase sums (the whole correction on the largest tap) to cost up to 6 dB at T = 512:
32 / 1023 had -54.8 dB where plain rounding gives -61.1 dB and the bound was -56.9 dB; with the correction spread over the largest
remainders it has -60.3 dB.  Captures at 1 / 2 and 1 / 32 are still received like native ones
(test_resample_emulated.py::test_capture_at_the_worst_ratios_is_received_like_a_native_one)."""
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


# ---- the whole design space (tests/resample_ref.py enumerates it without the library) ----------------------------------------------

import resample_ref as RR
from test_resample_emulated import emu  # noqa: F401  (the fixture: k0_pick_tile / k0_lds_bytes / k0_span of the device source)


@pytest.fixture(scope="module")
def designs():
    return RR.enumerate_designs()


def test_the_enumeration_is_the_space_the_header_describes(wm, designs):
    assert len(designs) == RR.N_DESIGNS
    assert {k[2] for k in designs} == set(range(16, 513, 16))                    # all 32 values of T
    assert sorted({k[0] for k in designs}) == list(range(1, 17)) + [18, 20, 22, 24, 25, 26, 28, 30, 32]
    assert max(k[1] for k in designs) == 1023
    assert max(k[0] / k[1] for k in designs) == 16.0
    # the library and the restated rule accept and refuse the same rates, Hz by Hz, around rates of every kind
    rng = np.random.default_rng(5)
    u = ctypes.c_uint
    for d in range(1, RR.MAX_DECIMATION + 1):
        near = [r[0] for k, rates in designs.items() for r in rates if r[1] == d]
        picks = [int(x) for x in rng.choice(near, 12)]
        rates = set(picks) | {x + 1 for x in picks} | {x - 1 for x in picks} | {int(x) for x in rng.integers(700000, 26000000 * d, 40)}
        for fin in rates:
            L_, M_, T_ = u(), u(), u()
            rc = wm.lib().wmbus_resampler_design(fin, 800000 * d, ctypes.byref(L_), ctypes.byref(M_), ctypes.byref(T_), None, 0)
            geo = RR.geometry(fin, d)
            if fin == 800000 * d:
                continue                                                         # the identity: no resampler at all
            assert (rc == 0) == (geo is not None), (fin, d)
            if geo:
                assert (L_.value, M_.value, T_.value) == geo, (fin, d)


def test_the_sample_and_the_corners_hit_every_T_and_every_L(designs):
    geos = [RR.geometry(f, d) for f, d in RR.CORNERS + RR.sample_designs()]
    assert all(g in designs for g in geos)
    assert {g[2] for g in geos} == {k[2] for k in designs} and len({g[2] for g in geos}) == 32
    assert {g[0] for g in geos} == {k[0] for k in designs} and len({g[0] for g in geos}) == 25


def highest_lds_index(L, M, T, tile):
    """The highest and lowest sample index the lane loop of k0_resample_block_t forms, restated from its expressions: a lane's first
    output is t0 = (w / L) 4 L + w % L for w < groups L, v = r0 + t0 M, b0 = sh + (T - 1) + v / L; it reads xs[b0 + i M - k] and
    xs[b0 + i M - k - 1] for i < 4 and even k < T.  Worst case r0 = L - 1, sh = 1."""
    groups = -(-tile // (4 * L))
    t_max = (groups - 1) * 4 * L + (L - 1) + 3 * L               # the last lane's fourth output = groups 4 L - 1
    assert t_max == groups * 4 * L - 1
    hi = 1 + (T - 1) + ((L - 1) + (groups - 1) * 4 * L * M + (L - 1) * M) // L + 3 * M
    # floor((r0 + t0 M) / L) + 3 M = floor((r0 + (t0 + 3 L) M) / L): the issue's form of the same index
    assert hi == 1 + (T - 1) + ((L - 1) + t_max * M) // L
    lo = 0 + (T - 1) + 0 - (T - 2) - 1                           # sh = 0, v = 0, i = 0, k = T - 2, the second read
    return hi, lo


def test_every_design_of_the_space(wm, emu, designs):
    """All 5750: geometry, exact phase sums, both accumulator bounds, the tile wmbus_open picks and its LDS, and the LDS span against
    the indices the lane loop forms.  Collects the designs that would meet one of wmbus_open's two refusals ('tile does not fit the
    LDS', 'accumulator bound for 16-bit input'): none does, the refusals are unreachable."""
    refused, small = [], {}
    for (L, M, T), rates in sorted(designs.items()):
        fin, d = rates[0]
        gL, gM, gT, taps = wm.resampler_design(fin, 800000 * d)
        assert (gL, gM, gT) == (L, M, T), (fin, d)
        t = taps.astype(np.int64)
        assert taps.shape == (L, T) and np.all(t.sum(axis=1) == 16384), (fin, d)
        worst = int(np.abs(t).sum(axis=1).max())
        assert 255 * worst + RR.BIAS < 2 ** 30, (fin, d)
        tile = emu.wm_emu_k0_pick_tile(L, M, T)
        lds = emu.wm_emu_k0_lds_bytes(L, M, T, tile) if tile else 0
        if 32768 * worst >= 2 ** 31 or tile == 0:
            refused.append((L, M, T, worst, tile))
            continue
        assert tile % (4 * L) == 0 and lds <= 65536, (L, M, T, tile, lds)
        small[tile] = small.get(tile, 0) + 1
        for tl in (tile, 190, 64):                               # the library's tile and the two the emulated tests use
            hi, lo = highest_lds_index(L, M, T, tl)
            span = emu.wm_emu_k0_span(L, M, T, tl)
            assert lo >= 0 and hi < span, (L, M, T, tl, hi, span)
            assert span - hi <= 3                                # and no slack beyond the rounding to a pair: the formula is the index
        # a lane's 32-bit v = r0 + t0 M
        assert (L - 1) + (tile + 4 * L) * M < 2 ** 32
    assert refused == [], refused
    assert min(small) == 128 and max(small) <= 2048
    # designs are a function of L / M alone: other rates of the same ratio give the same taps
    rng = np.random.default_rng(6)
    keys = sorted(designs)
    for i in rng.choice(len(keys), 60, replace=False):
        rates = designs[keys[i]]
        if len(rates) > 1:
            a, b = rates[0], rates[-1]
            assert np.array_equal(wm.resampler_design(a[0], 800000 * a[1])[3], wm.resampler_design(b[0], 800000 * b[1])[3])


# L / M -> (T, tile, LDS bytes) where the issue that asked for these corners states them
CORNER_GEOMETRY = {(32, 1023): (512, 128, None), (25, 799): (512, 200, None), (1, 32): (512, 480, 65356), (1, 31): (496, None, 65364),
                   (2, 63): (512, None, 65432), (3, 64): (352, 708, None), (32, 33): (32, None, None), (32, 63): (32, None, None),
                   (1, 2): (32, None, None), (1, 3): (48, None, None), (16, 1): (16, None, None), (8, 5): (16, None, None)}


@pytest.mark.parametrize("fin,d", RR.CORNERS, ids=RR.CORNER_IDS)
def test_corner_geometry(wm, emu, fin, d):
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    assert (L, M, T) == RR.geometry(fin, d)
    tile = emu.wm_emu_k0_pick_tile(L, M, T)
    lds = emu.wm_emu_k0_lds_bytes(L, M, T, tile)
    print(f"{fin} -> {800000 * d}: L / M = {L} / {M}, T = {T}, tile {tile}, LDS {lds} bytes, {-(-tile // (4 * L)) * L} of 256 lanes work")
    want = CORNER_GEOMETRY.get((L, M), (None, None, None))
    assert want[0] in (None, T) and want[1] in (None, tile) and want[2] in (None, lds)
    if (L, M) == (13, 16):
        assert all(RR.geometry(fin2, d2) is None or RR.geometry(fin2, d2)[0] != 13 for d2 in (1, 2, 3, 4) for fin2 in (800000 * d2 * 16 // 13,))


def stop_band_bound(stop_b_db, L, T, bins, margin_db):
    """Stop-band level of the float design combined IN AMPLITUDE with the rounding floor's expected peak: a Q14 rounding of +-0.5 LSB
    per tap is white with rms sqrt(T / 12 L) / 16384 relative to unity gain; its peak over `bins` bins is about sqrt(2 ln bins)
    times that (the peak of that many Rayleigh draws, taken generously: the bins of a 2^20-point transform of L T taps are not
    independent)."""
    k = math.sqrt(2.0 * math.log(bins))
    return 20 * math.log10(10 ** (stop_b_db / 20) + k * RR.rounding_floor(L, T)) + margin_db


def ripple_bound(ripple_b_db, L, T, margin_db):
    """The same in the pass band: |H| moves by at most the float design's deviation plus the floor's peak over the pass-band bins
    (fewer than 2^20 / 2 of them)."""
    k = math.sqrt(2.0 * math.log(N_BINS_PASS))
    return 20 * math.log10(10 ** (ripple_b_db / 20) + k * RR.rounding_floor(L, T)) + margin_db


N_BINS_PASS = RR.N_FFT // 2


def t_class(T):
    return "T = 16 .. 64" if T <= 64 else "T = 80 .. 240" if T <= 240 else "T = 256 .. 512"


def test_response_against_the_float_design(wm):
    """CORNERS + SAMPLE.  Three tap sets per design on the grid of the seven-rate test above: (a) the library's int16 taps, (b) an
    independent float64 prototype of the same (L, M, T) (tests/resample_ref.py::float_prototype), (c) the rounded scipy design.
    The reference is (b): ripple(a) and stop(a) must stay inside (b) combined in amplitude with the PREDICTED rounding floor
    (stop_band_bound / ripple_bound: nothing in them is fitted to (a)), plus a margin that is measured here, on (c) against (b) over
    the same designs: the worst excess of (c) over the prediction (never below 0) plus 1 dB for the stop band, plus 0.01 dB for the
    ripple.  (c) rounds like the library but leaves out its adjustment of each phase's largest tap.

    Measured on the default run: the margins come to 3.44 dB and 0.0101 dB; the envelope per class of T is in the module docstring.
    The seven rates above (T = 32 and 112, none of them with a whole M / L) keep 0.25 dB and -65 dB; the space as a whole does not."""
    rows = []
    for fin, d in RR.CORNERS + RR.sample_designs():
        fout = 800000 * d
        L, M, T, taps = wm.resampler_design(fin, fout)
        a = RR.response(taps.astype(np.float64) / 16384.0, L, M)
        b = RR.response(RR.float_prototype(L, M, T), L, M)
        c = RR.response(rounded_scipy_design(fin, fout, L, T) / 16384.0, L, M)
        rows.append((fin, d, L, M, T, a, b, c))
    margin_s = max(0.0, max(c[1] - stop_band_bound(b[1], L, T, b[2], 0.0) for _, _, L, M, T, a, b, c in rows)) + 1.0
    margin_r = max(0.0, max(c[0] - ripple_bound(b[0], L, T, 0.0) for _, _, L, M, T, a, b, c in rows)) + 0.01
    print(f"margins from the rounded scipy design: stop band {margin_s:.2f} dB, ripple {margin_r:.4f} dB")
    env = {}
    bad = []
    for fin, d, L, M, T, a, b, c in rows:
        sb, rb = stop_band_bound(b[1], L, T, b[2], margin_s), ripple_bound(b[0], L, T, margin_r)
        print(f"{fin} -> {800000 * d}: {L} / {M}, T = {T}: float {b[0]:.3f} dB, {b[1]:.1f} dB; int16 {a[0]:.3f} dB, {a[1]:.1f} dB; "
              f"scipy rounded {c[0]:.3f} dB, {c[1]:.1f} dB; bounds {rb:.3f} dB, {sb:.1f} dB")
        e = env.setdefault(t_class(T), [0.0, -999.0, 0.0, -999.0, 0])
        e[0], e[1], e[2], e[3], e[4] = max(e[0], b[0]), max(e[1], b[1]), max(e[2], a[0]), max(e[3], a[1]), e[4] + 1
        if a[0] > rb or a[1] > sb:
            bad.append((fin, d, L, M, T, a[:2], (rb, sb)))
    for cls, e in sorted(env.items()):
        print(f"{cls} ({e[4]} designs): float worst {e[0]:.3f} dB, {e[1]:.1f} dB; int16 worst {e[2]:.3f} dB, {e[3]:.1f} dB")
    assert bad == [], bad
