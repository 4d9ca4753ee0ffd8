"""The library's automatic frequency correction (include/wmbus_hip.h, AFC) restated in Python integers and numpy int64: the state a capture
carries from push to push, the plan of one push from the survey's accumulators, and the cu8 bytes the pipeline gets for a stream that is
cut into pushes.  The survey is tests/spectrum_ref.py's (the transform and the channel rule), the table, the rotation and the output
stage are tests/shift_ref.py's, the sample rules and the resampler's sum tests/format_ref.py's, the blocker tests/dc_ref.py's, the AGC
tests/agc_ref.py's.  All of them stay as they are; what is written out here is what AFC adds: range, hysteresis, step, base."""
import numpy as np

import agc_ref as AR
import dc_ref as DR
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR

RANGE_HZ = 64000                                    # cfg.input_afc_range_hz = 0
CAP = 8


def initial(nominal=0):
    return dict(held_hz=int(nominal), locked=0, changes=0, ratio_q8=0, base=0)


def hysteresis(fin):
    return fin // 256                               # two survey bins


def plan(fin, nominal, range_hz, st, total, peak, blocks, n_in):
    """One push of n_in input samples: the accumulators as they stand with this push included.  Returns (step, base of the push's first
    sample, the state behind the push)."""
    st = dict(st)
    range_hz = range_hz or RANGE_HZ
    hits = PR.channels(fin, total, peak, blocks, cap=CAP) or []
    cand = next((h for h in hits if abs(h["offset_hz"] - nominal) <= range_hz), None)
    if cand is not None and (not st["locked"] or abs(cand["offset_hz"] - st["held_hz"]) > hysteresis(fin)):
        st.update(held_hz=cand["offset_hz"], ratio_q8=cand["ratio_q8"], locked=1, changes=st["changes"] + 1)
    step = SR.step_of(fin, st["held_hz"])
    base = st["base"]
    st["base"] = (base + step * n_in) % (1 << 32)
    return step, base, st


def public(st):
    """What wmbus_read_input_afc returns of a state."""
    return dict(shift_hz=st["held_hz"], locked=st["locked"], changes=st["changes"], ratio_q8=st["ratio_q8"])


def accumulators(raw, fmt, cuts, R=0):
    """(sum, peak, blocks, n_in) behind every push of a stream: cuts = raw bytes per push."""
    pw = PR.power(PR.dft(PR.windowed(raw, fmt, R)))              # [level blocks, 512]
    out, off = [], 0
    for n in cuts:
        off += n
        blocks = off // FR.BPS[fmt] // PR.N
        out.append((pw[:blocks].sum(axis=0).astype(np.uint64), pw[:blocks].max(axis=0, initial=0).astype(np.uint32), blocks, n // FR.BPS[fmt]))
    assert off == raw.size
    return out


def plans(raw, fmt, fin, cuts, nominal=0, range_hz=0, R=0):
    """The plan of every push of a stream: cuts = raw bytes per push.  Returns a list of (step, base, state behind the push)."""
    out, st = [], initial(nominal)
    for total, peak, blocks, n_in in accumulators(raw, fmt, cuts, R):
        step, base, st = plan(fin, nominal, range_hz, st, total, peak, blocks, n_in)
        out.append((step, base, st))
    return out


def indices(script, n_samples):
    """Table index of every input sample: script = (step, base) per push, n_samples = input samples per push.  Sample j of a push has
    the phase (base + step j) mod 2^32."""
    idx = []
    for (step, base), n in zip(script, n_samples):
        phase = (np.uint64(base) + np.uint64(step) * np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)      # step j < 2^32 2^31
        idx.append((((phase + np.uint64(1 << 21)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64))
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def rotate(x, idx):
    """x int64 [n, 2] in front of the rotation (the 8-bit formats widened), idx the table index per sample: FREQUENCY SHIFT's rule."""
    cs = SR.table()[idx]
    c, s = cs[:, 0], cs[:, 1]
    a, b = x[:, 0] * c + x[:, 1] * s + 8192, x[:, 1] * c - x[:, 0] * s + 8192
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) < 2 ** 31
    return np.clip(np.stack([a >> 14, b >> 14], axis=1), -32768, 32767)


def convert(raw, fmt, cuts, script, R=0, agc=0, g_q8=256, L=1, M=1, taps=None):
    """The bytes of a whole stream whose pushes (cuts, raw bytes each) were rotated with script = (step, base) per push.  Returns (uint8
    [2 * n_out], bytes the clamp changed).  The blocker, the AGC's peak and the resampler do not know about pushes: they run over the
    stream; only the phase does."""
    x = FR.to_x(raw, fmt)
    if R:
        x = DR.block_dc(x, R)[0]
    g = AR.block_gain(x, fmt) if agc else None
    y = rotate(64 * x if fmt in (FR.CU8, FR.CS8) else x, indices(script, [n // FR.BPS[fmt] for n in cuts]))
    sh = SR.SHIFT_F[fmt] + 8
    acc = FR.accumulate(y, L, M, taps)
    if agc:
        newest = np.arange(acc.shape[0], dtype=np.int64) * M // L
        v = (acc * g[newest // AR.BLOCK][:, None] + (128 << sh)) >> sh
    else:
        v = (acc * (int(g_q8) if g_q8 else 256) + (128 << sh)) >> sh
    clipped = int(np.count_nonzero((v < 0) | (v > 255)))
    return np.clip(v, 0, 255).astype(np.uint8).reshape(-1), clipped


def run(raw, fmt, fin, cuts, nominal=0, range_hz=0, R=0, agc=0, g_q8=256, L=1, M=1, taps=None):
    """A whole stream through AFC.  Returns (bytes uint8, clipped, [(step, base, state) per push])."""
    pl = plans(raw, fmt, fin, cuts, nominal, range_hz, R)
    y, clipped = convert(raw, fmt, cuts, [(p[0], p[1]) for p in pl], R, agc, g_q8, L, M, taps)
    return y, clipped, pl


def pipeline_bytes(raw, fmt, fin, cuts, nominal=0, range_hz=0, **kw):
    """What the decoder behind AFC sees of a whole capture: the whole 4096-byte blocks; and the plans."""
    y, _, pl = run(raw, fmt, fin, cuts, nominal, range_hz, **kw)
    return y[:y.size // 4096 * 4096], pl


def bytes_per_push(y, fmt, cuts, L=1, M=1):
    """How many bytes of the stream's output y each push hands to the pipeline (whole 4096-byte blocks of remainder + new)."""
    out, n_in, n_out, rem = [], 0, 0, 0
    for n in cuts:
        n_in += n // FR.BPS[fmt]
        end = (n_in * L + M - 1) // M
        total = rem + 2 * (end - n_out)
        out.append(total // 4096 * 4096)
        rem, n_out = total % 4096, end
    return out
