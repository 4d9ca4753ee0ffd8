"""The survey that forgets (include/wmbus_hip.h, SPECTRUM AGE; cfg.input_spectrum_age = A) restated: the view of a capture behind a push
from the power of every level block of the stream, and AFC's plans over views.  The transform and the channel rule are
tests/spectrum_ref.py's, the plan of one push is tests/afc_ref.py's; both stay as they are.  What is written out here is what the age
adds: which level blocks are members of the view.  And the lock per channel (CHANNEL AFC; cfg.input_channel_afc_hz): AFC's rule once
per channel, with the channel's nominal and range, on the capture's survey -- a loop, no new arithmetic."""
import numpy as np

import afc_ref as AF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR


def stream_power(raw, fmt, R=0):
    """pw int64 [level blocks, 512] of a whole stream: SPECTRUM's, unchanged."""
    return PR.power(PR.dft(PR.windowed(raw, fmt, R)))


def members(K_last, A, K_reset=0):
    """The level blocks of the view behind a push whose last level block is K_last: K <= K_last with K >> A in {e_now - 1, e_now} and
    K >= K_reset.  A = 0: the survey never forgets."""
    if K_last < 0:
        return range(0)
    lo = max(((K_last >> A) - 1) << A, 0) if A else 0
    return range(max(lo, K_reset), K_last + 1)


def view(pw, K_last, A, K_reset=0):
    """(sum uint64 [512], peak uint32 [512], blocks): the view behind the push that ends with level block K_last."""
    m = members(K_last, A, K_reset)
    part = pw[m.start:m.stop] if len(m) else pw[:0]
    return part.sum(axis=0).astype(np.uint64), part.max(axis=0, initial=0).astype(np.uint32), len(m)


def apply_plan(slots, K_first, n_blk, A, e_keep, clear):
    """What a push does to two slots held as sets of level-block indices, given the host's plan for it (the library's k0_spec_age_plan):
    the slots in `clear` (bits) are emptied, then every level block of the push whose epoch is not below e_keep joins slot epoch & 1.
    The union of the slots must then be members(K_last, A)."""
    for s in range(2):
        if clear >> s & 1:
            slots[s].clear()
    for K in range(K_first, K_first + n_blk):
        if K >> A >= e_keep:
            slots[(K >> A) & 1].add(K)


def views(raw, fmt, cuts, A, R=0, resets=()):
    """(sum, peak, blocks, n_in) behind every push of a stream: cuts = raw bytes per push; resets = indices of pushes behind which the
    capture's view is read with reset."""
    pw = stream_power(raw, fmt, R)
    out, off, K_reset = [], 0, 0
    for i, n in enumerate(cuts):
        off += n
        blocks = off // FR.BPS[fmt] // PR.N
        out.append(view(pw, blocks - 1, A, K_reset) + (n // FR.BPS[fmt],))
        if i in resets:
            K_reset = blocks
    assert off == raw.size
    return out


def plans(raw, fmt, fin, cuts, A, nominal=0, range_hz=0, R=0, resets=()):
    """AFC's plan of every push on the view: a list of (step, base, state behind the push)."""
    out, st = [], AF.initial(nominal)
    for total, peak, blocks, n_in in views(raw, fmt, cuts, A, R, resets):
        step, base, st = AF.plan(fin, nominal, range_hz, st, total, peak, blocks, n_in)
        out.append((step, base, st))
    return out


def run(raw, fmt, fin, cuts, A, nominal=0, range_hz=0, R=0, agc=0, g_q8=256, L=1, M=1, taps=None, resets=()):
    """A whole stream through AFC on an ageing survey: (bytes uint8, clipped, [(step, base, state) per push])."""
    pl = plans(raw, fmt, fin, cuts, A, nominal, range_hz, R, resets)
    y, clipped = AF.convert(raw, fmt, cuts, [(p[0], p[1]) for p in pl], R, agc, g_q8, L, M, taps)
    return y, clipped, pl


def pipeline_bytes(raw, fmt, fin, cuts, A, nominal=0, range_hz=0, **kw):
    y, _, pl = run(raw, fmt, fin, cuts, A, nominal, range_hz, **kw)
    return y[:y.size // 4096 * 4096], pl


def channel_plan(fin, nominal, range_hz, st, total, peak, blocks, n_in):
    """AFC's plan of one push for one channel of a list: range 0 means the channel is fixed -- no search, the state stays at the
    channel's own Hz, the phase runs on."""
    if range_hz:
        return AF.plan(fin, nominal, range_hz, st, total, peak, blocks, n_in)
    st = dict(st)
    step, base = SR.step_of(fin, st["held_hz"]), st["base"]
    st["base"] = (base + step * n_in) % (1 << 32)
    return step, base, st


def channel_plans(raw, fmt, fin, cuts, hz, ranges, A=0, R=0, resets=()):
    """Per channel c of ONE capture the plan of every push: [channel][push] (step, base, state behind the push).  Every channel sees the
    capture's own survey (its view, with A)."""
    out = []
    for nominal, range_hz in zip(hz, ranges):
        pl, st = [], AF.initial(nominal)
        for total, peak, blocks, n_in in views(raw, fmt, cuts, A, R, resets):
            step, base, st = channel_plan(fin, nominal, range_hz, st, total, peak, blocks, n_in)
            pl.append((step, base, st))
        out.append(pl)
    return out


def two_tones(n_push=6, push_bytes=8 * 4096, seed=7):
    """The capture that shows what the age is for: cu8 at 1.6 MS/s, noise of sigma 0.004 of full scale, a tone of amplitude
    0.5 at +25 kHz in pushes 0-1, a tone of amplitude 0.1 at -20 kHz from push 2 on.  Returns (raw uint8, cuts)."""
    fin, n = 1600000, n_push * push_bytes // 2
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    x = 0.004 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    first = t < 2 * push_bytes // 2
    x = x + np.where(first, 0.5 * np.exp(2j * np.pi * 25000 / fin * t), 0.1 * np.exp(-2j * np.pi * 20000 / fin * t))
    iq = np.stack([x.real, x.imag], axis=1)
    raw = np.clip(np.round(iq * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    return raw, [push_bytes] * n_push
