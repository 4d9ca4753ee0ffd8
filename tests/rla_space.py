"""Designed slicer-bit streams for the run-length framer (TEST INFRASTRUCTURE; tests/README.md, "The run-length framer's
input space").  Every stream is hand-built raw bits, enumerated and not drawn; tests/test_rla_space_emulated.py runs them
through the kernel's source on the host and through tests/rla_ref.py, and asserts on rla_ref's event list that each family
really produced what it was built for.

How raw runs show behind the deglitcher, once both levels have lasted six samples or more:
  T1/C1 (three ones among six): the level rises at the third one and falls at the fourth zero: L raw ones show as L + 1
        high samples, L zeros as L - 1 low ones;
  S1    (newest | majority of three): it rises at once and falls at the third zero: L ones -> L + 2, L zeros -> L - 2.
A framer reset clears the raw history (rtl_wmbus.c:632,723), the sample that caused it included, and the level restarts low
whatever the filter said: behind a reset the first low run lasts until the third (T1/C1) or the first (S1) raw one."""
import numpy as np

CODE = ([int(b) for b in format(0x543D, "016b")], [int(b) for b in format(0x547696, "024b")])      # rtl_wmbus.c:97-103, oldest chip first
SPC = (8, 24)                                            # samples per chip of a framer fresh from reset
GROW = (1, 2)                                            # what a high run gains and a low run loses behind the deglitcher


def rle(runs, first=0):
    out, lv = [], first
    for r in runs:
        out.append(np.full(int(r), lv, np.uint8)); lv ^= 1
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def raw_runs(chain, druns, first=0):
    """raw run lengths that show as the deglitched runs `druns` (alternating, the first at level `first`) in a steady alternation"""
    g = GROW[chain]
    return [max(1, d - g) if (first ^ (i & 1)) else d + g for i, d in enumerate(druns)]      # (S1 has no high run of 2 or 3 samples, T1/C1 none below 4)


def kick(chain):
    """Behind a low stretch: three raw ones, a high pulse too short for either framer, and the zeros up to (not including)
    the sample at which the pulse's falling edge resets the framer."""
    return np.array([1, 1, 1, 0, 0, 0][:6 - chain], np.uint8)


def after_reset(chain, druns):
    """raw bits from the reset sample on that show as `druns`, the first of them the low run the reset sample begins"""
    first = druns[0] + (-2, 0)[chain]
    return rle([first] + raw_runs(chain, druns[1:], first=1), 0)


def cell(chain, druns, lead=16, tail=0):
    """a quiet lead, a forced reset, the designed deglitched runs, zeros"""
    return np.concatenate([np.zeros(lead, np.uint8), kick(chain), after_reset(chain, druns), np.zeros(tail, np.uint8)])


def pad_to(bits, mod, rem):
    return np.concatenate([bits, np.zeros((rem - len(bits)) % mod, np.uint8)])


def sweep(cells, mod=256):
    """each cell padded to a length of 1 modulo `mod` and repeated `mod` times: whatever a cell does, it does at every
    position of a step"""
    cells = [pad_to(c, mod, 1) for c in cells]
    return np.concatenate([c for c in cells for _ in range(mod)])


def chips_druns(chips, spc):
    runs = []
    for i, c in enumerate(chips):
        if i and c == chips[i - 1]: runs[-1] += spc
        else: runs.append(spc)
    return runs


# ---- T1/C1: deglitched runs from reset that bring the bit length to exactly 2 * 256 r + {0, 1, -1, -2}, r = 5..8, found by
# a best-first search over the tracker's update (rtl_wmbus.c:792-796) and checked here through rla_ref's events.  Key: (bit
# length, level of the run that follows).  A run of r samples is then exactly half a chip (reset, :756) or, from the two
# lengths below, half a chip and 1/256 sample (one chip).
_P5 = [12, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 12]
_P6 = [12, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 15, 15, 15, 16, 16, 17, 15]
_P7 = [12, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 15, 15, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20]
_P8 = [12, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 15, 15, 15, 16, 16, 17, 17, 18, 18, 19, 19, 20, 20, 21, 22, 22, 13]
HALF_PATHS = {
    (2560, 0): _P5 + [7, 28], (2560, 1): _P5 + [17], (2561, 0): _P5, (2561, 1): _P5 + [27],
    (2559, 0): _P5 + [26, 28], (2559, 1): _P5 + [7], (2558, 0): _P5 + [7, 17], (2558, 1): _P5 + [26],
    (3072, 0): _P6 + [19, 20, 20], (3072, 1): _P6, (3073, 0): _P6 + [20, 19, 20], (3073, 1): _P6 + [20, 19],
    (3071, 0): _P6 + [19], (3071, 1): _P6 + [20, 7], (3070, 0): _P6 + [7], (3070, 1): _P6 + [19, 19, 8, 8],
    (3584, 0): _P7 + [8, 8], (3584, 1): _P7 + [23], (3585, 0): _P7 + [23, 22], (3585, 1): _P7 + [23, 22, 8],
    (3583, 0): _P7 + [8, 22], (3583, 1): _P7 + [8, 22, 8], (3582, 0): _P7 + [8, 22, 8, 22], (3582, 1): _P7 + [8],
    (4096, 0): _P8 + [25, 25, 25], (4096, 1): _P8 + [25, 25], (4097, 0): _P8 + [25, 25, 9], (4097, 1): _P8 + [25, 25, 9, 25],
    (4095, 0): _P8 + [8, 9, 9], (4095, 1): _P8 + [25, 25, 25, 9], (4094, 0): _P8 + [25], (4094, 1): _P8 + [8, 9],
}


def half_chip_cell(bitlen, level):
    r = (bitlen + 2) // 512
    return cell(0, HALF_PATHS[(bitlen, level)] + [r, 12], tail=12)


def spb_path(want0, want1, level=None, limit=80):
    """S1: deglitched runs from reset (the first one low) that leave the two samples-per-bit trackers at (want0, want1) with a
    run of `level` to follow, by a breadth-first search over the rule (rtl_wmbus.c:655-698); None where the rule cannot get there."""
    start = (24, 24, 0)
    prev, queue = {start: None}, [start]
    while queue:
        nxt = []
        for st in queue:
            s0, s1, lv = st
            if (s0, s1) == (want0, want1) and level in (None, lv):
                path = []
                while prev[st] is not None:
                    st, d = prev[st]; path.append(d)
                return path[::-1]
            unit = (s0 + s1) // 2; half = unit // 2
            if unit <= 12 or unit >= 36: continue
            for d in range(half + 1, limit):
                n = (d - half + unit - 1) // unit
                to = (s0, d // n, 0) if lv else (d // n, s1, 1)
                if to not in prev:
                    prev[to] = (st, d); nxt.append(to)
        queue = nxt
    return None


# ---- the families ------------------------------------------------------------------------------------------------------------
def edge_position(chain):
    """every kind of edge of this chain, at either level, at every sample of a 256-sample step"""
    if chain == 0:
        return {"chips": rle([8, 9] * 300),
                "run<5 high": rle([10, 3] * 300),
                "run<5 low": sweep([np.concatenate([np.zeros(16, np.uint8), rle([10, 5, 10], 1)])]),
                "half a chip": sweep([half_chip_cell(2560, 0), half_chip_cell(2560, 1)])}
    return {"chips": rle([24, 25] * 270),
            "run0<=half": rle([8, 9] * 300),
            "spb low side": sweep([cell(1, [13, 13, 12, 20], tail=8), cell(1, [13, 13, 13, 12, 20], tail=8)]),
            "spb high side": sweep([cell(1, [36, 36, 20], tail=8), cell(1, [30, 36, 36, 20], tail=8)])}


def reset_patch(chain):
    """a reset at k = 58..63 of each word of a step, the five raw samples behind it taking all 32 values"""
    kk = kick(chain)
    cells = [(k, v) for k in range(58, 64) for v in range(32) for _ in range(4)]
    bits = np.zeros(64 * (len(cells) + 1), np.uint8)
    resets = []
    for i, (k, v) in enumerate(cells):
        p = 64 * i + k
        bits[p - len(kk):p] = kk
        bits[p + 1:p + 6] = [(v >> j) & 1 for j in range(5)]
        resets.append(p)
    return {"patch": bits}, resets


def de_bruijn(n):
    """the binary de Bruijn sequence of order n (Lyndon words, lexicographically least)"""
    a, seq = [0] * (n + 1), []

    def db(t, p):
        if t > n:
            if n % p == 0: seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, 2):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    return np.array(seq, np.uint8)


def deglitch_seams():
    """The order-11 de Bruijn sequence with one more zero in its run of zeros: 2049 bits that hold every 11-bit window (and
    every 8-bit one) cyclically.  2049 = 1 modulo 256, so 256 periods put every window at every sample of a step: across every
    half word, word and step at every alignment."""
    s = de_bruijn(11)
    period = np.concatenate([[0], s]).astype(np.uint8)               # the sequence starts with its eleven zeros
    return {"de Bruijn 11": np.tile(period, 257)[:2049 * 256 + 10]}


def chip_counts_t1(settle=(6, 7, 8, 9, 10, 11, 12), runs=range(5, 401)):
    """the tracker settled on chips of c samples (sixty runs of c), then every run of 5..400 samples, two runs of c between
    them and sixty behind a run short enough to reset the framer"""
    out = {}
    for c in settle:
        d = [c] * 60
        for L in runs:
            d += [L] + [c] * (60 if 512 * L <= 256 * c + 512 else 2)
        if len(d) % 2: d.append(c)
        out["settled on %d" % c] = cell(0, d, tail=8)
    return out


S1_PAIRS = ((13, 13), (35, 35), (24, 24), (13, 35), (35, 13), (18, 30), (30, 18))


def chip_counts_s1(pairs=S1_PAIRS, runs=range(1, 301)):
    """the two samples-per-bit trackers brought to a pair from reset, then every run of 1..300 samples at either level"""
    out = {}
    for a, b in pairs:
        paths = [spb_path(a, b, lv) for lv in (0, 1)]
        if None in paths: continue
        cells = [cell(1, path + [L, 20], tail=8) for L in runs for path in paths]
        out["spb %d/%d" % (a, b)] = np.concatenate(cells)
    return out


LONG_T1 = (list(range(180, 213)) + list(range(1012, 1037, 4)),                                      # n = 23..26; 32 n = 4064..4128
           (65524, 65528, 65532, 65533, 65534, 65535, 65536, 65537, 65541, 65545), (65534, 65535, 65536, 65537))   # low; high
LONG_S1 = (list(range(552, 640, 3)), (106489, 106496, 106509))        # unit 24: n = 23..26; unit 13: 8191, 8192, 8193 chips, each leaving 13 samples per bit


def long_runs(chain):
    """long runs at the shift cap, at the chip limit, at 2^24 and at 32 n = 4096, each followed at once by the access code"""
    sp, out = SPC[chain], {}
    pre = [sp] * 6                                                       # a few chips from reset; the next run is low
    def one(L, level, spc, lead):
        code = chips_druns(CODE[chain][1:] if level == 0 else CODE[chain], spc)
        return cell(chain, lead + ([] if level == 0 else [spc]) + [L] + code + [spc], tail=12)
    if chain == 0:
        out["short"] = np.concatenate([one(L, lv, 8, pre) for L in LONG_T1[0] for lv in (0, 1)])
        out["2^24 low"] = np.concatenate([one(L, 0, 8, pre) for L in LONG_T1[1]])
        out["2^24 high"] = np.concatenate([one(L, 1, 8, pre) for L in LONG_T1[2]])
    else:
        out["short"] = np.concatenate([one(L, lv, 24, pre) for L in LONG_S1[0] for lv in (0, 1)])
        p13 = spb_path(13, 13, 0)                                        # the long run low
        out["chip limit"] = np.concatenate([one(L, 0, 13, p13) for L in LONG_S1[1]])
    return out


def access_code(chain):
    code, sp = CODE[chain], SPC[chain]
    pre = [0, 1] * 4
    body = lambda chips: cell(chain, chips_druns(chips, sp) + [sp], tail=12)
    every_k = np.concatenate([pad_to(body(pre + code), 64, 1) for _ in range(64)])
    miss = [body(pre + [c ^ (i == j) for j, c in enumerate(code)]) for i in range(len(code))]
    return {"marker at every k": every_k,
            "behind a reset": np.concatenate([body(code), body(code)]),
            "near misses": np.concatenate(miss),
            "back to back": body(pre + code + code)}


def ragged_base():
    """a stream with something of everything (chips, both reset rules, an access code now and then) for the ragged pushes"""
    parts = []
    for i in range(520):
        parts.append(rle([8, 9] * (3 + i % 5) + [3, 11] * (i % 3) + [24, 25] * (i % 4)))
        if i % 9 == 0: parts.append(access_code(i // 9 % 2)["behind a reset"][:600])
    return np.concatenate(parts)


def ragged_pushes():
    """push lengths: ending at every residue of a step (so of a word), runs of pushes that each end 1..4 samples into a
    word, and pushes of 1..5 samples"""
    a = [256 + r for r in range(1, 256)]
    b = [64 * j + e for e in (1, 2, 3, 4) for j in (0, 1, 3, 4, 0, 0, 2, 5)]
    c = [1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    return a, b, c


STAGING_CAP = (80, 32)                                   # the primary region (chips) the staging streams are built around, per chain


def staging(chain, seg_len=1024):
    """1024-sample segments whose chip counts on `chain` run through every value in STAGING_CAP[chain] - 8 .. + 8 (and
    beyond): a varying number of one-chip runs, then a stretch that gives few chips of its own"""
    parts = []
    if chain == 0:
        for i in range(150):                             # T1/C1: 67..91 chips a segment
            body = rle([8, 9] * (4 + i % 25) + [8] * (i // 25 % 2))
            fill = seg_len - len(body)
            parts.append(np.concatenate([body, rle([5, 3] * (fill // 8 + 2))[i % 7:][:fill]]))
    else:
        for i in range(200):                             # S1: 23..41 chips a segment (the body is too fast for it, the stretch one long run)
            body = rle([8, 9] * (8 + (i * 7) % 19))
            fill = seg_len - len(body) - 24 * (i % 4) - 3 * (i % 3)
            parts.append(np.concatenate([body, np.tile(np.array([1, 0], np.uint8), fill // 2), np.zeros(seg_len - len(body) - fill // 2 * 2, np.uint8)]))
    return np.concatenate(parts)
