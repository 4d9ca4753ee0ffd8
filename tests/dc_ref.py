"""The library's integer I/Q DC blocker (include/wmbus_hip.h, next to wmbus_read_input_dc) restated in numpy int64 and Python integers:
raw bytes of cu8 / cs8 / cs16 / cf32 in, the cu8 bytes the pipeline gets out, for a context with cfg.input_dc = R.  The level sums,
the recurrence, the rounding of dc and the saturating subtraction are written out here; the sample rules and the resampler's sum are
tests/format_ref.py's, the rotation and the 16-bit scale of the 8-bit formats under a shift are tests/shift_ref.py's.  Both stay as they
are."""
import numpy as np

import format_ref as FR
import shift_ref as SR

BLOCK = 512                                         # input samples per level block


def recurrence(S, R):
    """S: the level sums of one component, in order.  Returns dc per block, Python integers throughout (>> floors)."""
    assert 1 <= R <= 12
    dc, A = [], None
    for v in S:
        v = int(v)
        A = (v << R) if A is None else A - (A >> R) + v
        dc.append(min(max((A + (1 << (8 + R))) >> (9 + R), -32768), 32767))
    return dc


def block_dc(x, R):
    """x int64 [n, 2], n a multiple of 512: the int16 samples by the unshifted rules.  Returns (x' int64 [n, 2], dc int64 [n / 512, 2])."""
    x = np.asarray(x, np.int64)
    assert x.ndim == 2 and x.shape[1] == 2 and x.shape[0] % BLOCK == 0
    S = x.reshape(-1, BLOCK, 2).sum(axis=1)
    assert np.abs(S).max(initial=0) <= 1 << 24
    dc = np.stack([np.array(recurrence(S[:, c], R), np.int64).reshape(-1) for c in (0, 1)], axis=1).reshape(-1, 2)
    return np.clip(x - np.repeat(dc, BLOCK, axis=0), -32768, 32767), dc


def convert(raw, fmt, R, fin=0, f=0, g_q8=256, L=1, M=1, taps=None):
    """Returns (uint8 [2 * n_out], number of bytes the clamp changed, dc int64 [n / 512, 2]).  f != 0: the frequency shift of
    tests/shift_ref.py at the input rate fin behind the blocker."""
    g = int(g_q8) if g_q8 else 256
    assert 1 <= g <= 65535
    x, dc = block_dc(FR.to_x(raw, fmt), R)
    if f:
        x = SR.rotate(64 * x if fmt in (FR.CU8, FR.CS8) else x, SR.step_of(fin, f))
        sh = SR.SHIFT_F[fmt] + 8
    else:
        sh = FR.SHIFT_F[fmt] + 8
    v = (FR.accumulate(x, L, M, taps) * g + (128 << sh)) >> sh
    clipped = int(np.count_nonzero((v < 0) | (v > 255)))
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1), clipped, dc


def pipeline_bytes(raw, fmt, R, fin=0, f=0, g_q8=256, L=1, M=1, taps=None):
    """What the decoder behind the blocker sees of a whole capture: the whole 4096-byte blocks."""
    y = convert(raw, fmt, R, fin, f, g_q8, L, M, taps)[0]
    return y[:y.size // 4096 * 4096]


def add_offset_cu8(cu8, d_i, d_q):
    """A constant (d_i, d_q) added to every cu8 byte pair, clipped to 0 ... 255: what a zero-IF front end's offset does to a capture.
    d_i, d_q: scalars or one value per sample."""
    u = np.asarray(cu8, np.uint8).reshape(-1, 2).astype(np.int64)
    u[:, 0] += d_i
    u[:, 1] += d_q
    return np.clip(u, 0, 255).astype(np.uint8).reshape(-1)
