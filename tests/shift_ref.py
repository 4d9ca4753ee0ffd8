"""The library's integer frequency shift (include/wmbus_hip.h, next to wmbus_shift_design) restated in numpy int64 and Python
integers: raw bytes of cu8 / cs8 / cs16 / cf32 in, the cu8 bytes the pipeline gets out, for a context with cfg.input_shift_hz.  The
resampler's taps come from the library (taps=None: the input is at decimation x 800 kHz already); the step, the table, the
rotation, the 16-bit scale of the 8-bit formats and the output stage are written out here.  tests/format_ref.py is the case without
a shift and stays as it is; its sample rules and its resampler sum are used, nothing of its output stage."""
import numpy as np

import format_ref as FR

ENTRIES = 1024
SHIFT_F = {FR.CU8: 21, FR.CS8: 21, FR.CS16: 22, FR.CF32: 22}


def step_of(fin, f):
    """floor((f 2^32 + Fin / 2) / Fin) mod 2^32 in Python integers (// floors, also for negative f)."""
    assert 2 * abs(f) <= fin
    return ((f << 32) + fin // 2) // fin % (1 << 32)


def table():
    """int64 [1024, 2]: {c, s} = rint(16384 cos / sin(2 pi i / 1024)), in double."""
    w = 2.0 * np.pi * np.arange(ENTRIES) / ENTRIES
    return np.stack([np.rint(16384.0 * np.cos(w)), np.rint(16384.0 * np.sin(w))], axis=1).astype(np.int64)


def indices(step, m0, n):
    """Table index of the samples m0 .. m0 + n of the stream.  step m < 2^64 while m < 2^32: uint64 holds it; beyond that Python
    integers."""
    if m0 + n <= 1 << 32:
        phase = (np.uint64(step) * np.arange(m0, m0 + n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
        return (((phase + np.uint64(1 << 21)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
    return np.array([((((step * m) % (1 << 32)) + (1 << 21)) % (1 << 32)) >> 22 for m in range(m0, m0 + n)], np.int64)


def to_x(raw, fmt):
    """int64 [n, 2]: the sample in front of the rotation -- the 8-bit formats widened to 16 bits."""
    x = FR.to_x(raw, fmt)
    return 64 * x if fmt in (FR.CU8, FR.CS8) else x


def rotate_wide(x, step, m0=0):
    """x int64 [n, 2] = (xi, xq) of the stream's samples m0 ...; returns int64 [n, 2] in front of the clamp to int16."""
    cs = table()[indices(step, m0, x.shape[0])]
    c, s = cs[:, 0], cs[:, 1]
    xi, xq = x[:, 0], x[:, 1]
    a, b = xi * c + xq * s + 8192, xq * c - xi * s + 8192
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) < 2 ** 31      # the kernel's products and sums are int32
    return np.stack([a >> 14, b >> 14], axis=1)


def rotate(x, step, m0=0):
    """The rotated samples y, int64 [n, 2]."""
    return np.clip(rotate_wide(x, step, m0), -32768, 32767)


def rotation_clamps(raw, fmt, fin, f, m0=0):
    """How many components the rotation's clamp to int16 changes."""
    w = rotate_wide(to_x(raw, fmt), step_of(fin, f), m0)
    return int(np.count_nonzero((w < -32768) | (w > 32767)))


def convert(raw, fmt, fin, f, g_q8=256, L=1, M=1, taps=None, m0=0):
    """Returns (uint8 [2 * n_out], number of bytes the clamp changed).  m0: index of raw's first sample within the stream (everything
    in front of it rotates to y = 0, like the history before a stream)."""
    g = int(g_q8) if g_q8 else 256
    assert 1 <= g <= 65535
    y = rotate(to_x(raw, fmt), step_of(fin, f), m0)
    sh = SHIFT_F[fmt] + 8
    v = (FR.accumulate(y, L, M, taps) * g + (128 << sh)) >> sh
    clipped = int(np.count_nonzero((v < 0) | (v > 255)))
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1), clipped


def pipeline_bytes(raw, fmt, fin, f, g_q8=256, L=1, M=1, taps=None):
    """What the decoder behind the shift sees of a whole capture: the whole 4096-byte blocks."""
    y = convert(raw, fmt, fin, f, g_q8, L, M, taps)[0]
    return y[:y.size // 4096 * 4096]


def mixed_up(cu8, fin, f):
    """The cu8 capture as complex z = (2u - 255), mixed UP by f in double: z e^(+j 2 pi f m / Fin), what a receiver whose channel lies
    f above its centre would have recorded, before quantisation.  The turn count f m mod Fin is reduced in integers."""
    u = np.asarray(cu8, np.uint8).reshape(-1, 2).astype(np.float64)
    z = (2.0 * u[:, 0] - 255.0) + 1j * (2.0 * u[:, 1] - 255.0)
    turns = (int(f) * np.arange(z.size, dtype=np.int64)) % int(fin)
    return z * np.exp(2j * np.pi * (turns.astype(np.float64) / fin))


def round_trip_cs16(cu8, fin, f):
    """rint(90 z') as cs16 raw bytes; decoded with input_shift_hz = f and input_gain_q8 = 364 it is the capture again."""
    z = 90.0 * mixed_up(cu8, fin, f)
    return FR.raw_bytes(np.rint(np.stack([z.real, z.imag], axis=1)).reshape(-1).astype(np.int16), FR.CS16)


def round_trip_cu8(cu8, fin, f):
    """u = clip(rint((z' / 1.45 + 255) / 2)) as cu8 raw bytes; decoded with input_shift_hz = f and input_gain_q8 = 371."""
    z = mixed_up(cu8, fin, f) / 1.45
    return np.clip(np.rint((np.stack([z.real, z.imag], axis=1).reshape(-1) + 255.0) / 2.0), 0, 255).astype(np.uint8)


CS16_ROUND_TRIP_GAIN = 364                          # floor(256 * 128 / 90)
CU8_ROUND_TRIP_GAIN = 371
