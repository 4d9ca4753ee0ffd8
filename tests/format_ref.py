"""The library's sample formats and input gain (include/wmbus_hip.h, next to wmbus_resampler_design) restated in numpy int64: raw
bytes of cu8 / cs8 / cs16 / cf32 in, the cu8 bytes the pipeline gets out.  The taps come from the library (taps=None: the input is
at decimation x 800 kHz already, the filter is the delta acc = 16384 x); everything else is written out here.  Whole stream in,
every output byte out.  tests/resample_ref.py is the cu8, gain x 1 case of this and stays as it is."""
import numpy as np

CU8, CS8, CS16, CF32 = 0, 1, 2, 3
NAMES = {CU8: "cu8", CS8: "cs8", CS16: "cs16", CF32: "cf32"}
BPS = {CU8: 2, CS8: 2, CS16: 4, CF32: 8}                # raw bytes per IQ sample
SHIFT_F = {CU8: 15, CS8: 15, CS16: 22, CF32: 22}
SILENCE = {CU8: 128, CS8: 0, CS16: 0, CF32: 0}          # the byte that pads an ended stream with "no signal"


def raw_bytes(values, fmt):
    """Sample values (uint8 / int8 / int16 / float32, I and Q interleaved) as the raw little-endian bytes the library takes."""
    dt = {CU8: "u1", CS8: "i1", CS16: "<i2", CF32: "<f4"}[fmt]
    return np.ascontiguousarray(np.asarray(values).astype(dt, copy=False)).view(np.uint8).reshape(-1)


def to_x(raw, fmt):
    """raw: uint8 bytes.  Returns int64 [n, 2]: the int16 sample x per I and Q."""
    raw = np.ascontiguousarray(raw, np.uint8)
    if fmt == CU8:
        x = 2 * raw.astype(np.int64) - 255
    elif fmt == CS8:
        x = 2 * raw.view(np.int8).astype(np.int64) + 1
    elif fmt == CS16:
        x = raw.view("<i2").astype(np.int64)
    elif fmt == CF32:
        with np.errstate(invalid="ignore", over="ignore"):       # (signalling NaNs among random bit patterns)
            f = raw.view("<f4").astype(np.float64)               # f * 32768 is exact in double; nothing is lost against float
            v = np.where(np.isnan(f), 0.0, f * 32768.0)
            x = np.clip(np.rint(np.clip(v, -32768.0, 32767.0)), -32768, 32767).astype(np.int64)   # rint: round half even
    else:
        raise ValueError(fmt)
    assert x.min(initial=0) >= -32768 and x.max(initial=0) <= 32767
    return x.reshape(-1, 2)


def n_outputs(n_in, L, M):
    return (n_in * L + M - 1) // M


def accumulate(x, L, M, taps):
    """acc [n_out, 2] int64: the resampler's sum (history before the stream: x = 0); taps None: 16384 x."""
    if taps is None:
        return 16384 * x
    T = taps.shape[1]
    xx = np.concatenate([np.zeros((T - 1, 2), np.int64), x])
    n = np.arange(n_outputs(x.shape[0], L, M), dtype=np.int64)
    p, b = (n * M) % L, (n * M) // L + (T - 1)
    h = taps.astype(np.int64)
    acc = np.zeros((n.size, 2), np.int64)
    for k in range(T):
        acc += h[p, k][:, None] * xx[b - k]
    assert np.abs(acc).max(initial=0) < 2 ** 31                  # the kernel's accumulator is an int32
    return acc


def convert(raw, fmt, g_q8=256, L=1, M=1, taps=None):
    """Returns (uint8 [2 * n_out], number of bytes the clamp changed)."""
    g = int(g_q8) if g_q8 else 256
    assert 1 <= g <= 65535
    sh = SHIFT_F[fmt] + 8
    v = (accumulate(to_x(raw, fmt), L, M, taps) * g + (128 << sh)) >> sh
    clipped = int(np.count_nonzero((v < 0) | (v > 255)))
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1), clipped


def pipeline_bytes(raw, fmt, g_q8=256, L=1, M=1, taps=None):
    """What the decoder behind the conversion sees of a whole capture: the whole 4096-byte blocks."""
    y = convert(raw, fmt, g_q8, L, M, taps)[0]
    return y[:y.size // 4096 * 4096]


def embed(cu8, fmt):
    """A cu8 capture written in another format so that, at gain x 1, it converts back to the very same bytes."""
    u = np.asarray(cu8, np.uint8).astype(np.int64)
    if fmt == CU8:
        return raw_bytes(u.astype(np.uint8), CU8)
    if fmt == CS8:
        return raw_bytes((u - 128).astype(np.int8), CS8)
    if fmt == CS16:
        return raw_bytes((128 * (2 * u - 255)).astype(np.int16), CS16)
    if fmt == CF32:
        return raw_bytes(((2 * u - 255) / 256.0).astype(np.float32), CF32)       # exact: nine significant bits
    raise ValueError(fmt)
