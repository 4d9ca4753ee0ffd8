"""The library's channel activity (include/wmbus_hip.h, CHANNEL ACTIVITY) restated in Python integers: the rule that turns one pipeline
row's power timeline P (tests/power_ref.py) into a record per burst of energy, and the matching of a line to its burst.  Every division
floors.  Also the constructed timelines the rule, the emulated kernel and the GPU tests share."""
import numpy as np

EPOCH = 64
QUARTILE = 16
DEFAULT_T = 1024


def epochs_back(fin):
    """H = min(63, ceil(0.16 Fin / 32768) + 1)."""
    return min(63, -(-fin // 204800) + 1)


def rule(p, fin, T=0):
    """[dict(first_block, blocks, mean, floor)] of the timeline p = P of level blocks 0, 1, ... of one row."""
    T = T or DEFAULT_T
    p = [int(v) for v in p]
    H = epochs_back(fin)
    n_ep = len(p) // EPOCH                                      # the last incomplete epoch is never evaluated
    q = [sorted(p[EPOCH * e:EPOCH * (e + 1)])[QUARTILE] for e in range(n_ep)]
    floor = [min(q[max(0, e - H):e + 1]) for e in range(n_ep)]
    act = [p[K] * 256 > T * floor[K >> 6] for K in range(EPOCH * n_ep)]
    out, K = [], 0
    while K < len(act):
        if not act[K]:
            K += 1
            continue
        first = K
        while K < len(act) and act[K]:
            K += 1
        if K < len(act) and K - first >= 2:                     # closed by an inactive block of a complete epoch
            out.append(dict(first_block=first, blocks=K - first, mean=sum(p[first:K]) // (K - first), floor=floor[first >> 6]))
    return out


def matches(burst, ka):
    """first_block - 1 <= ka < first_block + blocks."""
    return burst["first_block"] - 1 <= ka < burst["first_block"] + burst["blocks"]


def match(bursts, ka):
    """The index of the burst (of the line's row) that a line with access-code level block ka belongs to, or -1."""
    hits = [i for i, b in enumerate(bursts) if matches(b, ka)]
    assert len(hits) <= 1, "bursts of a row are disjoint"
    return hits[0] if hits else -1


def strip(records):
    """The rule's four fields of library records."""
    return [dict(first_block=r["first_block"], blocks=r["blocks"], mean=r["mean"], floor=r["floor"]) for r in records]


# ---- constructed timelines --------------------------------------------------------------------------------------------------------------

def runs_timeline(n, runs, low=1000, high=9000, seed=0):
    """n level blocks of `low` (+ a little seeded variation, far below any threshold used), with every (first, blocks) of `runs` at `high`."""
    rng = np.random.default_rng(seed)
    p = (low + rng.integers(0, low // 8 + 1, n)).astype(np.uint32) if low else np.zeros(n, np.uint32)
    for first, blocks in runs:
        p[first:first + blocks] = high
    return p


def cases(fin=1600000):
    """{name: (P uint32, fin, T)}: every case the issue names, each a whole stream."""
    H = epochs_back(fin)
    c = {}
    c["all_equal"] = (np.full(64 * 4, 777, np.uint32), fin, 0)                                     # ties in the quartile, nothing active
    flat = np.zeros(64 * 3, np.uint32)
    flat[[5, 6, 7, 20, 64, 65, 130]] = [3, 1, 2, 9, 4, 4, 8]
    c["floor_zero"] = (flat, fin, 0)                                                               # floor 0: any P > 0 is active
    c["len_1_and_2"] = (runs_timeline(64 * 3, [(10, 1), (20, 2), (63, 1), (70, 1), (100, 2)]), fin, 0)
    c["lane_0_and_63"] = (runs_timeline(64 * 4, [(64, 5), (120, 8), (190, 2), (254, 2)]), fin, 0)   # starts in lane 0; ends in lane 63 (twice)
    c["two_epochs"] = (runs_timeline(64 * 4, [(60, 10), (127, 2)]), fin, 0)
    c["three_epochs"] = (runs_timeline(64 * 5, [(50, 100)]), fin, 0)
    c["whole_epoch_inside"] = (runs_timeline(64 * 6, [(100, 64 * 2 + 30)]), fin, 0)                 # an epoch wholly inside a run does not lift the floor
    long = runs_timeline(64 * (H + 6), [])
    long[:64] = 400                                                                                # a quiet first epoch: the floor holds it for H epochs more, then forgets
    long[64 * 2::7] = 1800                                                                         # x 4.5 over 400, x 1.8 over 1000: runs of one while the floor remembers
    for first, blocks in ((70, 4), (64 * (H + 3) + 9, 5)):
        long[first:first + blocks] = 5000
    c["floor_forgets"] = (long, fin, 0)
    carrier = runs_timeline(64 * (H + 8), [(100, 64 * (H + 8) - 100)], high=20000)
    c["carrier"] = (carrier, fin, 0)                                                               # closes by itself once the floor holds it
    c["h_clamp"] = (runs_timeline(64 * 70, [(64 * 1 + 3, 64 * 66)], high=7000), 12800000, 0)       # H = 63 at 12.8 MS/s
    edge = np.full(64 * 3, 1024, np.uint32)
    edge[[10, 11, 12, 40, 41]] = [1029, 1029, 1028, 4096, 4097]                                    # x 257 / 256 = 1028: 1029 active, 1028 not; x 4: 4097 active, 4096 not
    for T in (257, 1024, 65535):
        c[f"T_{T}"] = (edge.copy(), fin, T)
    big = edge.copy()
    big[[70, 71, 72]] = [262141, 262140, 262141]                                                   # x 65535 / 256 = 262140: 262141 active, 262140 not -> runs of one
    big[[80, 81]] = 262141
    c["T_65535_hits"] = (big, fin, 65535)
    c["trailing"] = (runs_timeline(64 * 3 + 37, [(30, 6), (64 * 3 - 3, 10), (64 * 3 + 20, 5)]), fin, 0)   # the run across the last complete epoch's end is never closed
    rng = np.random.default_rng(7)
    noisy = rng.integers(900, 1300, 64 * 9 + 11).astype(np.uint32)
    for first in rng.integers(0, noisy.size - 40, 14):
        noisy[first:first + int(rng.integers(1, 40))] += np.uint32(rng.integers(2000, 9000))
    c["random"] = (noisy, fin, 0)
    return c


CUTS = (1, 3, 64, 5, 67)                            # pushes of these many level blocks in turn


def cut(n, units=CUTS):
    """[(start, stop)] covering n level blocks, the push sizes cycling through `units`."""
    out, at, i = [], 0, 0
    while at < n:
        step = min(units[i % len(units)], n - at)
        out.append((at, at + step)); at += step; i += 1
    return out
