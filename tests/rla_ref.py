"""The run-length framer, restated sample by sample (TEST INFRASTRUCTURE): rtl_wmbus.c:640-702 (S1) and :729-803 (T1/C1) as
the reference runs them -- one raw slicer bit in, the shift register, the deglitch table, the edge test, the reset rules, the
chip count-down, the trackers -- with no bit tricks and no knowledge of words, steps, segments or pushes.  What the kernel
(rtl-wmbus_amd/csrc/wm_k2_rla.h) computes 256 samples at a time must be what this computes one sample at a time: the chips,
the framer state at any sample, and which segments saw an access code.

The divisions here are Python's integers, truncated towards zero as C does; the operands of every one of them are kept in
the event list, so a test can say which corners of wm_udiv its input reached."""
import numpy as np

RUN_LIMIT = 8192                                          # WM_RLA_RUN_LIMIT: chips materialised per edge
SYNC = (0x543D, 0x547696)                                 # rtl_wmbus.c:97-103
SYNC_MASK = (0xFFFF, 0xFFFFFF)
# rtl_wmbus.c:126-144: ones among the last six raw bits >= 3; :149-154: newest | majority of the three before
DEGLITCH_T1C1 = [int(bin(i).count("1") >= 3) for i in range(64)]
DEGLITCH_S1 = [0, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1]

CHIPS, RST_RUN5, RST_HALF, RST_SPB, RST_RUN0 = "chips", "run<5", "runq<=half", "spb", "run0<=half"
KINDS = ((CHIPS, RST_RUN5, RST_HALF), (CHIPS, RST_SPB, RST_RUN0))      # per chain
STATE_FIELDS = ("run", "bitlen", "cum", "state", "raw", "sr", "spb0", "spb1")


def cdiv(a, b):
    """C's a / b for b > 0"""
    return -((-a) // b) if a < 0 else a // b


def reset_state(pending=False):
    """runlength_algorithm_reset_* (:628-637, :717-726); `pending`: the next chip is the first one behind a reset"""
    return dict(run=0, bitlen=8 * 256, cum=0, level=0, pending=int(pending), raw=0, sr=0, spb0=24, spb1=24)


def canonical(chain, s):
    """The state as WmRlaState holds it: raw = the last five raw bits in time order (T1/C1; the S1 table looks back three
    samples, kept in place), sr masked to the access code's width."""
    in_time_order = sum(((s["raw"] >> j) & 1) << (4 - j) for j in range(5))      # the reference shifts left: its bit 0 is the newest, the record's bit 4
    return dict(run=s["run"], bitlen=s["bitlen"], cum=s["cum"], state=s["level"] | (s["pending"] << 1),
                raw=in_time_order & (0x1C if chain else 0x1F), sr=s["sr"] & SYNC_MASK[chain], spb0=s["spb0"], spb1=s["spb1"])


class Result:
    def __init__(self):
        self.runs = []          # (sample, first value, level, kept chips, rssi byte) per chip-run edge
        self.events = []        # dict(sample, kind, n, run, div) per edge; div: the (dividend, divisor) pairs of its divisions
        self.states = {}        # requested sample -> canonical state BEFORE that sample is taken in
        self.final = None       # the state behind the last sample, to carry into the next call

    def chips(self, rssi=False):
        """[(sample, value)] (with rssi: a third column), at most RUN_LIMIT chips per edge"""
        cols = 3 if rssi else 2
        if not self.runs:
            return np.zeros((0, cols), np.uint32)
        r = np.array(self.runs, np.int64)
        first = np.concatenate([[0], np.cumsum(r[:-1, 3])])
        idx = np.repeat(np.arange(len(r)), r[:, 3])
        out = np.stack([r[idx, 0], r[idx, 2]] + ([r[idx, 4]] if rssi else []), axis=1)
        out[first, 1] = r[:, 1]
        return out.astype(np.uint32)

    def marker_samples(self):
        return [r[0] for r in self.runs if r[1] & 2]


def run(chain, bits, rssi=None, start=None, at=(), origin=0, trace=None):
    """One chain (0: T1/C1, 1: S1) over `bits`.  start: the state dict of an earlier call's .final (default: a fresh
    context, no reset pending).  at: samples (counted from `origin`, the sample number of bits[0]) whose state is wanted.
    trace: a list that receives one text line per sample, the fields of the reference's struct runlength_algorithm_* behind
    that sample as oracle/ref_probe.c's mode `rla` writes them: run length; bit length and cumulative error, or the two
    samples-per-bit; level; the raw register's 6 (4) newest bits; the chip register masked to the access code."""
    s = dict(start) if start is not None else reset_state()
    res = Result()
    want = set(int(a) for a in at)
    lut = DEGLITCH_S1 if chain else DEGLITCH_T1C1
    win = 0xF if chain else 0x3F
    sync, mask = SYNC[chain], SYNC_MASK[chain]
    bl = np.asarray(bits, np.uint8).tolist()
    n_bits = len(bl)
    raw, level, run_ = s["raw"], s["level"], s["run"]
    mid = lambda: f' {s["spb0"]} {s["spb1"]} ' if chain else f' {s["bitlen"]} {s["cum"]} '
    tail, middle = f' {s["sr"] & mask}\n', mid()
    for i in range(n_bits):
        if want and origin + i in want:
            s["raw"], s["level"], s["run"] = raw, level, run_
            res.states[origin + i] = canonical(chain, s)
        raw = ((raw << 1) | bl[i]) & 0x3F
        st = lut[raw & win]
        if st == level:
            run_ += 1
            if trace is not None: trace.append(f"{run_}{middle}{level} {raw & win}{tail}")
            continue
        # ---- an edge of the deglitched signal ----
        m = origin + i
        ev = dict(sample=m, level=level, run=run_, n=0, div=())
        kind = None
        if not chain:
            unit = s["bitlen"]; half = cdiv(unit, 2); runq = run_ * 256
            if run_ < 5: kind = RST_RUN5                                      # :742
            elif runq <= half: kind = RST_HALF                                # :756
        else:
            unit = cdiv(s["spb0"] + s["spb1"], 2); half = cdiv(unit, 2); runq = run_
            if unit <= 12 or unit >= 36: kind = RST_SPB                       # :659
            elif run_ <= half: kind = RST_RUN0                                # :671
        ev["unit"], ev["half"] = unit, half
        if kind is not None:
            s = reset_state(pending=True)
            raw = 0
        else:
            kind = CHIPS
            left, n, first, sr = runq, 0, None, s["sr"]
            while left > half:                                                # :765-779 / :680-694
                left -= unit
                sr = ((sr << 1) | level) & 0xFFFFFFFF
                chip = level | (2 if (sr & mask) == sync else 0)
                if n == 0:
                    first = chip | (s["pending"] << 2)
                else:
                    assert not chip & 2                                       # the chips of a run are equal: only its first can end the code
                n += 1
                if n >= 64 and left > half:                                   # the rest of a long run, in one go: the register is all `level` by now
                    more = cdiv(left - half + unit - 1, unit)
                    left -= more * unit; n += more
                    sr = mask if level else 0
            s["sr"] = sr
            s["pending"] = 0
            res.runs.append((m, first, level, min(n, RUN_LIMIT), 0 if rssi is None else min(255, int(rssi[i]))))
            if not chain:
                s["cum"] += left                                              # :792-796
                num = left + cdiv(s["cum"], 16)
                s["bitlen"] += cdiv(num, 32 * n)
                ev["div"] = ((runq - half + unit - 1, unit), (num, 32 * n))
            else:
                s["spb1" if level else "spb0"] = cdiv(run_, n)                # :698
                ev["div"] = ((runq - half + unit - 1, unit), (run_, n))
            ev["n"] = n
        ev["kind"] = kind
        res.events.append(ev)
        level = st
        run_ = 1
        if trace is not None:
            tail, middle = f' {s["sr"] & mask}\n', mid()
            trace.append(f"{run_}{middle}{level} {raw & win}{tail}")
    s["raw"], s["level"], s["run"] = raw, level, run_
    res.final = s
    if want and origin + n_bits in want:
        res.states[origin + n_bits] = canonical(chain, s)
    return res
