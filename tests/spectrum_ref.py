"""The library's channel survey (include/wmbus_hip.h, SPECTRUM) restated: the exact integer 512-point windowed DFT per level block in numpy
int64, vectorised over blocks, with the sum and the max-hold per bin; and the channel rule of wmbus_spectrum_channels in Python integers.
The sample rules are tests/format_ref.py's, the DC blocker is tests/dc_ref.py's, the {c, s} table is tests/shift_ref.py's; everything else
is written out here."""
import numpy as np

import dc_ref as DR
import format_ref as FR
import shift_ref as SR

N = 512                                             # points = input samples of a level block = bins
STAGES = 9


def window():
    """int64 [512]: w[n] = (16384 - c[2 n] + 1) >> 1, a Hann window in Q14."""
    c = SR.table()[:, 0]
    return (16384 - c[2 * np.arange(N)] + 1) >> 1


def bitrev():
    n = np.arange(N)
    r = np.zeros(N, np.int64)
    for k in range(STAGES):
        r |= ((n >> k) & 1) << (STAGES - 1 - k)
    return r


def windowed(raw, fmt, R=0):
    """y int64 [blocks, 512, 2]: the windowed samples of every level block; R: cfg.input_dc."""
    x = FR.to_x(raw, fmt)
    assert x.shape[0] % N == 0
    if R:
        x = DR.block_dc(x, R)[0]
    v = 64 * x if fmt in (FR.CU8, FR.CS8) else x
    assert np.abs(v).max(initial=0) <= 32768
    y = (v.reshape(-1, N, 2) * window()[None, :, None] + 8192) >> 14
    assert y.min(initial=0) >= -32768 and y.max(initial=0) <= 32767
    return y


def dft(y):
    """z int64 [blocks, 512, 2]: bit reversal, then the nine radix-2 decimation-in-time stages with the rotation's rounding."""
    cs = SR.table()
    z = y[:, bitrev(), :].copy()
    for s in range(1, STAGES + 1):
        half = 1 << (s - 1)
        g = z.reshape(z.shape[0], N >> s, 2, half, 2)            # [block, group, a | b, j, re | im]
        i = np.arange(half) * (1024 >> s)
        c, sn = cs[i, 0][None, None, :], cs[i, 1][None, None, :]
        a, b = g[:, :, 0], g[:, :, 1]
        t = np.stack([(b[..., 0] * c + b[..., 1] * sn + 8192) >> 14, (b[..., 1] * c - b[..., 0] * sn + 8192) >> 14], axis=-1)
        z = np.stack([a + t, a - t], axis=2).reshape(z.shape[0], N, 2)
        assert np.abs(z).max(initial=0) < 2 ** 31                # the kernel's z is int32
    return z


def power(z):
    """pw int64 [blocks, 512] in BIN order: bin b = (j + 256) mod 512 <-> (b - 256) Fin / 512."""
    pw = (z[..., 0] * z[..., 0] + z[..., 1] * z[..., 1]) >> 16
    assert pw.max(initial=0) < 2 ** 32
    return np.roll(pw, N // 2, axis=1)


def spectrum(raw, fmt, R=0):
    """(sum uint64 [512], peak uint32 [512], blocks) of a whole stream of raw bytes (whole level blocks)."""
    pw = power(dft(windowed(raw, fmt, R)))
    return pw.sum(axis=0).astype(np.uint64), pw.max(axis=0, initial=0).astype(np.uint32), pw.shape[0]


def bin_hz(fin):
    return (np.arange(N) - N // 2) * fin / N


# ---- the channel rule ------------------------------------------------------------------------------------------------------------

WIDTH_HZ, MIN_RATIO_Q8, REL = 200000, 1024, 8       # the defaults for 0


def channels(in_hz, total, peak, blocks, width_hz=0, min_ratio_q8=0, rel=0, cap=64):
    """The list of hits, dicts of offset_hz, ratio_q8, floor_peak, floor_mean; None where the library returns WMBUS_EINVAL.  Python
    integers throughout (// floors, also for negative numerators)."""
    width_hz, min_ratio_q8, rel = width_hz or WIDTH_HZ, min_ratio_q8 or MIN_RATIO_Q8, rel or REL
    if in_hz < 800000 or blocks == 0 or min_ratio_q8 < 257:
        return None
    peak = [int(v) for v in peak]
    total = [int(v) for v in total]
    W = min(max(width_hz * N // in_hz, 1), 256)
    Fp = max(1, sorted(peak)[255])
    Fm = max(1, sorted(v // blocks for v in total)[255])
    B = [sum(peak[b:b + W]) for b in range(N - W + 1)]
    alive = [True] * len(B)
    e = [max(0, v - Fp) for v in peak]
    hits, first = [], None
    while len(hits) < cap:
        best = None
        for b in range(len(B)):
            if alive[b] and (best is None or B[b] > B[best]):
                best = b
        if best is None or B[best] * 256 < min_ratio_q8 * W * Fp or (first is not None and B[best] * rel < first):
            break
        if first is None:
            first = B[best]
        lo = best
        for trip in range(3):
            d = sum(e[lo:lo + W])
            if d == 0:                                           # cannot happen on the first trip (min_ratio_q8 > 256); later: keep the last window
                break
            den, num = d, sum(e[i] * (i - 256) for i in range(lo, lo + W))
            cb = (2 * num + den) // (2 * den)
            nlo = min(max(cb + 256 - W // 2, 0), N - W)
            if nlo == lo:
                break
            lo = nlo
        hits.append(dict(offset_hz=(2 * num * in_hz + N * den) // (2 * N * den), ratio_q8=min(B[best] * 256 // (W * Fp), 2 ** 32 - 1),
                         floor_peak=Fp, floor_mean=Fm))
        for b in range(len(B)):
            if abs(b - best) < W:
                alive[b] = False
    return hits


def strongest_ratio_q8(in_hz, peak, width_hz=0):
    """B 256 / (W Fp) of the strongest window: what the threshold is held against."""
    peak = [int(v) for v in peak]
    W = min(max((width_hz or WIDTH_HZ) * N // in_hz, 1), 256)
    Fp = max(1, sorted(peak)[255])
    return max(sum(peak[b:b + W]) for b in range(N - W + 1)) * 256 // (W * Fp)
