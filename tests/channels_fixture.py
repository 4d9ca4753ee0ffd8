"""Shared by tests/test_channels_emulated.py and tests/test_gpu_channels.py: the three-channel wideband capture the channels tests decode,
and the per-channel restatement.  Nothing here defines arithmetic: a channel of a multi-channel context is a single-shift context, so
tests/shift_ref.py, dc_ref.py and agc_ref.py are the oracle, per channel."""
import numpy as np

import agc_ref as AR
import dc_ref as DR
import format_ref as FR
import shift_ref as SR

WIDE_FS = 4000000                                   # 4.0 MS/s: L / M / T = 2 / 5 / 48 to 1.6 MS/s
WIDE_HZ = [700000, -600000, 0]                      # where the three captures sit in the wideband one
WIDE_N = 1 << 19                                    # samples
WIDE_GAIN = 409                                     # Q8; 819 clips, 409 and 273 do not
WIDE_SCALE = 40
WIDE_LINES = [8, 10, 6]                             # lines of each capture alone = of its channel: counted on the CPU (the floor below is 6)


def wideband(wm, hz=None):
    """(cs16 raw bytes of the sum of three synthetic 4.0 MS/s captures mixed to WIDE_HZ, scaled x 40, rounded, clipped to int16; the three
    cu8 captures).  hz: other offsets for the three (the same captures with their channels swapped)."""
    z, parts = 0.0, []
    for i, f in enumerate(hz or WIDE_HZ):
        cu8, _ = wm.synth_capture(seed=9100 + i, n_samples=WIDE_N, fs_khz=WIDE_FS // 1000, kinds=15, frames_per_s=60.0)
        parts.append(cu8)
        z = z + SR.mixed_up(cu8, WIDE_FS, f)
    v = np.clip(np.rint(WIDE_SCALE * np.stack([z.real, z.imag], axis=1)), -32768, 32767).astype(np.int16)
    return FR.raw_bytes(v.reshape(-1), FR.CS16), parts


def restated(raw, fmt, fin, f, g_q8=256, L=1, M=1, taps=None, R=0, agc=0):
    """(bytes, clip count, dc table or None, gain table or None) of ONE channel: what a single-shift context with input_shift_hz = f gives.
    f = 0 takes the restatements' unshifted branch under the blocker or the AGC -- a 0 Hz channel goes through the rotating rule with
    step 0 in the library, which must give the same bytes -- and shift_ref's rotating rule otherwise."""
    if agc:
        y, clips, g = AR.convert(raw, fmt, R, fin, f, L, M, taps)
        dc = DR.block_dc(FR.to_x(raw, fmt), R)[1] if R else None
        return y, clips, dc, g
    if R:
        y, clips, dc = DR.convert(raw, fmt, R, fin, f, g_q8, L, M, taps)
        return y, clips, dc, None
    y, clips = SR.convert(raw, fmt, fin, f, g_q8, L, M, taps)
    return y, clips, None, None


def whole_blocks(y):
    return y[:y.size // 4096 * 4096]
