"""The library's per-block integer AGC (include/wmbus_hip.h, next to wmbus_read_input_gain) restated in numpy int64: raw bytes of cu8 /
cs8 / cs16 / cf32 in, the cu8 bytes the pipeline gets out, for a context with cfg.input_agc = 1.  The peak, the division, the clamp
of g and which g an output takes are written out here; the sample rules and the resampler's sum are tests/format_ref.py's, the rotation
and the 16-bit scale of the 8-bit formats under a shift are tests/shift_ref.py's, the blocker in front is tests/dc_ref.py's.  All three
stay as they are."""
import numpy as np

import dc_ref as DR
import format_ref as FR
import shift_ref as SR

BLOCK = 512                                         # input samples per level block: the DC blocker's
TARGET = 96                                         # where a block's peak |I| + |Q| lands, of the byte's +-127
U = {FR.CU8: 9, FR.CS8: 9, FR.CS16: 16, FR.CF32: 16}


def gain_of(P, fmt):
    """g of one level block from its peak P = max(|x'_I| + |x'_Q|), Python integers."""
    P = int(P)
    assert 0 <= P <= 65536
    return min(max((TARGET << U[fmt]) // max(P, 1), 1), 65535)


def block_gain(x, fmt):
    """x int64 [n, 2], n a multiple of 512: the int16 samples by the unshifted rules, behind the blocker where there is one.
    Returns g int64 [n / 512]."""
    x = np.asarray(x, np.int64)
    assert x.ndim == 2 and x.shape[1] == 2 and x.shape[0] % BLOCK == 0
    P = (np.abs(x[:, 0]) + np.abs(x[:, 1])).reshape(-1, BLOCK).max(axis=1)
    return np.array([gain_of(p, fmt) for p in P], np.int64)


def convert(raw, fmt, R=0, fin=0, f=0, L=1, M=1, taps=None):
    """Returns (uint8 [2 * n_out], number of bytes the clamp changed, g int64 [n / 512]).  R != 0: the DC blocker of tests/dc_ref.py in
    front; f != 0: the frequency shift of tests/shift_ref.py at the input rate fin behind the peak (the peak is taken of x', unrotated)."""
    x = FR.to_x(raw, fmt)
    if R:
        x = DR.block_dc(x, R)[0]
    g = block_gain(x, fmt)
    if f:
        x = SR.rotate(64 * x if fmt in (FR.CU8, FR.CS8) else x, SR.step_of(fin, f))
        sh = SR.SHIFT_F[fmt] + 8
    else:
        sh = FR.SHIFT_F[fmt] + 8
    acc = FR.accumulate(x, L, M, taps)
    newest = np.arange(acc.shape[0], dtype=np.int64) * M // L        # the newest input sample of output n
    assert newest.max(initial=0) < x.shape[0]
    v = (acc * g[newest // BLOCK][:, None] + (128 << sh)) >> sh
    clipped = int(np.count_nonzero((v < 0) | (v > 255)))
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1), clipped, g


def pipeline_bytes(raw, fmt, R=0, fin=0, f=0, L=1, M=1, taps=None):
    """What the decoder behind the AGC sees of a whole capture: the whole 4096-byte blocks."""
    y = convert(raw, fmt, R, fin, f, L, M, taps)[0]
    return y[:y.size // 4096 * 4096]
