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


# ---- the design space (include/wmbus_hip.h: L <= 32, M <= 1024, in_hz >= 800000, T = 16 max(1, ceil(M / L)) <= 512), restated
# without the library: nothing below calls it.
import math
import os

MAX_L, MAX_M, MAX_T, MAX_DECIMATION = 32, 1024, 512, 16
N_DESIGNS = 5750                                    # distinct (L, M) over decimation 1 .. 16, identity excluded


def geometry(in_hz, decimation):
    """(L, M, T) of the resampler the header promises for this input rate and decimation; None: refused (or no resampler)."""
    out_hz = 800000 * decimation
    if in_hz < 800000 or in_hz == out_hz:
        return None
    g = math.gcd(in_hz, out_hz)
    L, M = out_hz // g, in_hz // g
    T = 16 * max(1, -(-M // L))
    return (L, M, T) if L <= MAX_L and M <= MAX_M and T <= MAX_T else None


def enumerate_designs():
    """{(L, M, T): [(in_hz, decimation), ...]} of every valid design.  L / M in lowest terms equals 800000 d / in_hz exactly when
    L divides 800000 d and in_hz = 800000 d / L * M, so the rates of a decimation are walked by (L, M), not Hz by Hz."""
    out = {}
    for d in range(1, MAX_DECIMATION + 1):
        for L in range(1, MAX_L + 1):
            if (800000 * d) % L:
                continue
            for M in range(1, MAX_M + 1):
                if math.gcd(L, M) != 1:
                    continue
                geo = geometry(800000 * d // L * M, d)
                if geo is not None:
                    assert geo[:2] == (L, M)
                    out.setdefault(geo, []).append((800000 * d // L * M, d))
    return out


# (in_hz, decimation): the corners of the space.  L / M, T and why are in tests/README.md; tile and LDS bytes are asserted in
# test_resampler_design.py::test_corner_geometry
CORNERS = [(825000, 1), (1650000, 2),               # 32 / 33: largest L
           (3150000, 2),                            # 32 / 63: largest L, T = 32
           (25575000, 1),                           # 32 / 1023: T = 512, the smallest tile (128 outputs: 32 of 256 lanes work)
           (25568000, 1),                           # 25 / 799: T = 512, tile 200
           (25600000, 1),                           # 1 / 32: T = 512, LDS 65 356 bytes
           (24800000, 1),                           # 1 / 31: T = 496, LDS 65 364 bytes
           (25200000, 1),                           # 2 / 63: T = 512, LDS 65 432 bytes, the largest of this list
           (51200000, 3),                           # 3 / 64: T = 352
           (3200000, 2), (2400000, 1),              # 1 / 2, 1 / 3: integer decimation
           (800000, 16),                            # 16 / 1: smallest T, pure upsampling
           (1000000, 2),                            # 8 / 5: upsampling
           (12800000, 13)]                          # 13 / 16: an L that exists only through the decimation
CORNER_IDS = [f"{f}-d{d}" for f, d in CORNERS]


def sample_designs(n_extra=None, seed=None):
    """A seeded draw from the enumeration, [(in_hz, decimation)]: one design for every value of T and one for every value of L that
    occurs (so that, whatever the seed, every T and every L is hit), then WMBUS_RESAMPLE_N (default 8) further ones drawn
    uniformly.  WMBUS_RESAMPLE_SEED moves the draw."""
    n_extra = int(os.environ.get("WMBUS_RESAMPLE_N", "8")) if n_extra is None else n_extra
    seed = int(os.environ.get("WMBUS_RESAMPLE_SEED", "0")) if seed is None else seed
    rng = np.random.default_rng(0xD351 + seed)
    designs = enumerate_designs()
    keys = sorted(designs)
    picked = []
    for field in (2, 0):                            # T, then L
        for value in sorted({k[field] for k in keys}):
            have = [k for k in keys if k[field] == value]
            picked.append(have[int(rng.integers(len(have)))])
    picked += [keys[int(i)] for i in rng.choice(len(keys), size=min(n_extra, len(keys)), replace=False)]
    corners = {geometry(f, d) for f, d in CORNERS}
    out, seen = [], set(corners)
    for k in picked:
        if k not in seen:
            seen.add(k)
            rates = designs[k]
            out.append(rates[int(rng.integers(len(rates)))])
    return out


def float_prototype(L, M, T):
    """The design in float64, independently of the library and of scipy: Kaiser-windowed sinc (beta 8) of L T taps at the prototype
    rate, cut-off 0.45 min(1, L / M) / L of it (the taps depend on L / M alone), every phase scaled to sum 1.  Returns [L, T]."""
    N = L * T
    t = np.arange(N) - (N - 1) / 2.0
    h = np.sinc(2.0 * 0.45 * min(1.0, L / M) / L * t) * np.kaiser(N, 8.0)
    ph = h.reshape(T, L).T
    return ph / ph.sum(axis=1, keepdims=True)


N_FFT = 1 << 20


def response(phases, L, M):
    """(pass-band ripple dB, stop-band peak dB, stop-band bins) of phases [L, T] scaled to sum 1 each, on the grid of
    test_resampler_design.py: FFT of 2^20, ripple up to 0.35 min(in, out), stop band from 0.6 min(in, out).  Frequencies are in units
    of the prototype rate L in_hz: in = 1 / L, out = 1 / M."""
    h = np.asarray(phases, np.float64).T.reshape(-1) / L
    H = np.abs(np.fft.rfft(h, N_FFT))
    f = np.arange(H.size) / N_FFT
    lo = min(1.0 / L, 1.0 / M)
    pb, sb = H[f <= 0.35 * lo], H[f >= 0.6 * lo]
    return float(np.abs(20 * np.log10(pb)).max()), float(20 * np.log10(max(sb.max(), 1e-12))), int(sb.size)


def rounding_floor(L, T):
    """rms of the response error that rounding every tap to Q14 (+-0.5 LSB, uniform) adds, relative to unity gain."""
    return math.sqrt(T / (12.0 * L)) / 16384.0


def blocks_input(L, M, bps, blocks=3, min_raw_blocks=5):
    """Raw bytes (a multiple of 4096, at least min_raw_blocks of them so that the uneven cut has three parts) that resample to at
    least `blocks` whole 4096-byte blocks."""
    n_in = -(-(2048 * blocks) * M // L)              # outputs n < n_in L / M exist: 2048 blocks of them need n_in >= 2048 blocks M / L
    raw = max(min_raw_blocks, -(-n_in * bps // 4096)) * 4096
    assert n_outputs(raw // bps, L, M) * 2 // 4096 >= blocks
    return raw


def cuts_for(raw_bytes):
    """The three cuts of a stream of raw_bytes: one push, the uneven cut (3 blocks, 1 block, the rest), every push 4096 bytes."""
    nb = raw_bytes // 4096
    assert nb >= 5 and raw_bytes % 4096 == 0
    return {"one": [raw_bytes], "uneven": [3 * 4096, 4096, (nb - 4) * 4096], "each-4096": [4096] * nb}


def resample_long(cu8, L, M, taps, chunk=1 << 15):
    """resample() for captures of hundreds of megabytes: the same sums phase by phase as float64 matrix products.  Every product
    and partial sum is an integer below 2^31, so float64 holds each exactly whatever the order: the bytes are those of resample()
    (test_resample_emulated.py::test_long_restatement_equals_the_plain_one)."""
    T = taps.shape[1]
    u = np.asarray(cu8, np.uint8).reshape(-1, 2)
    n_out = n_outputs(u.shape[0], L, M)
    out = np.empty((n_out, 2), np.uint8)
    h = taps.astype(np.float64)[:, ::-1]                                   # window order: oldest input first
    for p in range(L):
        # outputs n = n0 + j L have the phase (n0 M) % L for every j; their newest inputs lie M apart
        n0 = next((n for n in range(L) if (n * M) % L == p), None)
        if n0 is None or n0 >= n_out:
            continue
        count = (n_out - n0 + L - 1) // L
        for j0 in range(0, count, chunk):
            j1 = min(count, j0 + chunk)
            first = (n0 + j0 * L) * M // L - (T - 1)                       # oldest input of the chunk's first output
            last = (n0 + (j1 - 1) * L) * M // L
            x = np.zeros((last - first + 1, 2), np.float64)
            lo = max(first, 0)
            x[lo - first:] = 2.0 * u[lo:last + 1] - 255.0
            for c in range(2):
                col = np.ascontiguousarray(x[:, c])
                win = np.lib.stride_tricks.as_strided(col, shape=(j1 - j0, T), strides=(M * col.strides[0], col.strides[0]))
                acc = (win @ h[p]).astype(np.int64)
                out[n0 + j0 * L:n0 + j1 * L:L, c] = np.clip((acc + BIAS) >> 15, 0, 255)
    return out.reshape(-1)
