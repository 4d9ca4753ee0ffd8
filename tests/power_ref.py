"""The library's channel power (include/wmbus_hip.h, CHANNEL POWER) restated in numpy and Python integers on top of tests/spectrum_ref.py's
pw: the band rows of every level block (the waterfall), the channel window of a pipeline row, the row's power timeline P, and the rule that
turns a timeline into a line's record.  Every division floors."""
import numpy as np

import spectrum_ref as PR

BANDS = 32
WIDTH_HZ = 200000
SIM_HZ = 325000                                     # cfg.simultaneous: T1/C1 above the stage's centre, S1 below
U32 = 2 ** 32 - 1


def band_rows(raw, fmt, R=0):
    """uint32 [blocks, 32]: bp[K][j] = min(sum of pw[K][16 j .. 16 j + 16), 2^32 - 1)."""
    pw = PR.power(PR.dft(PR.windowed(raw, fmt, R)))              # int64, bin order
    return np.minimum(pw.reshape(-1, BANDS, PR.N // BANDS).sum(axis=2), U32).astype(np.uint32)


def window(fin):
    """(W, nb)."""
    W = min(max(WIDTH_HZ * PR.N // fin, 1), 256)
    return W, min(BANDS, -(-W // 16) + 1)


def centre(fin, f_hz):
    """(cb, lo, j0) of the window centred on f_hz (the chain's +-325 kHz of cfg.simultaneous included by the caller)."""
    W, nb = window(fin)
    cb = 256 + (1024 * f_hz + fin) // (2 * fin)
    lo = min(max(cb - W // 2, 0), PR.N - W)
    return cb, lo, min(lo >> 4, BANDS - nb)


def chain_hz(chain, simultaneous):
    return (SIM_HZ if chain == 0 else -SIM_HZ) if simultaneous else 0


def channel_power(rows, fin, f_hz):
    """uint32 [blocks]: P[K] = min(sum of bp[K][j0 .. j0 + nb), 2^32 - 1) for a row centred on f_hz."""
    nb = window(fin)[1]
    j0 = centre(fin, f_hz)[2]
    return np.minimum(rows[:, j0:j0 + nb].astype(np.int64).sum(axis=1), U32).astype(np.uint32)


def guard(fin):
    """(G, Nn): the 10 ms in front of the access code that may hold the preamble, and the 20 ms of the noise window, in level blocks."""
    return -(-fin // 51200), -(-fin // 25600)


def history(fin):
    """Level blocks of P a context keeps in front of the current push."""
    G, Nn = guard(fin)
    return Nn + G + -(-(3 * fin) // 10240)                       # ceil(0.15 Fin / 512)


def block_of(sample, decimation=2, L=1, M=1):
    """m(n) >> 9, m(n) = floor(n D M / L): the level block of the raw input that decimated sample n stands for."""
    return (int(sample) * decimation * M // L) >> 9


def ratio_lm(in_hz, out_hz):
    """L / M of the resampler in lowest terms (out_hz / in_hz)."""
    from math import gcd
    g = gcd(in_hz, out_hz)
    return out_hz // g, in_hz // g


def line_record(p, first_block, ka, ke, fin):
    """The record of a line whose access code lies in level block ka and whose completing chip in ke, from p = P of level blocks
    first_block, first_block + 1, ...; a level block outside p is missing, like K < 0."""
    p = [int(v) for v in p]
    end = first_block + len(p)
    G, Nn = guard(fin)
    sig = [p[K - first_block] for K in range(max(ka + 1, first_block), min(ke, end))]
    noi = sorted(p[K - first_block] for K in range(max(ka - G - Nn, 0, first_block), min(max(ka - G, 0), end)))
    signal = sum(sig) // len(sig) if sig else 0
    noise = noi[len(noi) // 4] if noi else 0
    if not sig or not noi:
        ratio = 0
    elif noise == 0:
        ratio = U32 if signal > 0 else 0
    else:
        ratio = min(signal * 256 // noise, U32)
    return dict(first_block=ka, signal=signal, noise=noise, ratio_q8=ratio, n_signal=min(len(sig), 65535), n_noise=min(len(noi), 65535))
