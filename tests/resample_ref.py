"""The library's exact integer resampler (include/wmbus_hip.h, wmbus_resampler_design) restated in numpy int64: the taps come
from the library, everything else is written out here.  Whole stream in, every output byte out."""
import numpy as np

BIAS = 255 * 16384 + 16384


def n_outputs(n_in, L, M):
    """Outputs that exist once n_in input samples are in: output n needs input floor(n M / L)."""
    return (n_in * L + M - 1) // M


def resample(cu8, L, M, taps):
    """cu8: uint8 [2 * n_in] (I, Q interleaved); taps: int16 [L, T].  Returns uint8 [2 * n_out]."""
    T = taps.shape[1]
    u = np.asarray(cu8, np.uint8).reshape(-1, 2).astype(np.int64)
    x = np.concatenate([np.zeros((T - 1, 2), np.int64), 2 * u - 255])      # history before the stream: u = 127.5
    n = np.arange(n_outputs(u.shape[0], L, M), dtype=np.int64)
    p, b = (n * M) % L, (n * M) // L + (T - 1)                             # phase, newest input (index into x)
    h = taps.astype(np.int64)
    acc = np.zeros((n.size, 2), np.int64)
    for k in range(T):
        acc += h[p, k][:, None] * x[b - k]
    assert np.abs(acc).max(initial=0) < 2 ** 23
    return np.clip((acc + BIAS) >> 15, 0, 255).astype(np.uint8).reshape(-1)


def pipeline_bytes(cu8, L, M, taps):
    """What the decoder behind the resampler sees of a whole capture: the whole 4096-byte blocks."""
    y = resample(cu8, L, M, taps)
    return y[:y.size // 4096 * 4096]
