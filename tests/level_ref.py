"""The line levels (cfg.line_levels) restated in numpy: include/wmbus_hip.h, LINE LEVELS, is the definition; this file says the same
in Python integers (arbitrary precision, floor division), so nothing here can overflow or round.  TEST INFRASTRUCTURE."""
import numpy as np

CHAIN_T1C1, CHAIN_S1 = 0, 1
LO = {CHAIN_T1C1: 256, CHAIN_S1: 782}
HI = {CHAIN_T1C1: 128, CHAIN_S1: 586}
TAIL = 782                                           # soft symbols a context carries per (chain, capture)
QMAX = 1 << 20


def quantise(s):
    """q = clamp(rint(s 2^20), -2^20, 2^20) as int64; the product is exact in f32 (or +-inf), rint rounds half to even, NaN -> 0."""
    s = np.asarray(s, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(s * np.float32(QMAX))            # float32 throughout
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, -QMAX, QMAX))
    return v.astype(np.int64)


def level(dphi, a, chain):
    """The record for access-code sample `a` (global decimated index) of `chain` on the chain's soft symbols dphi[0 .. ) from the stream's
    first sample on: dict(sync_sample, offset_hz, dev_hz, n)."""
    lo, hi = LO[chain], HI[chain]
    a = int(a)
    if a - lo < 0:
        return dict(sync_sample=a, offset_hz=0, dev_hz=0, n=0)
    n = lo - hi
    q = [int(x) for x in quantise(dphi[a - lo:a - hi])]
    assert len(q) == n
    total = sum(q)
    mean = (2 * total + n) // (2 * n)
    adev = sum(abs(x - mean) for x in q)
    return dict(sync_sample=a, offset_hz=(total * 3125 + n * 4096) // (n * 8192), dev_hz=(adev * 3125 + n * 4096) // (n * 8192), n=n)


def sync_chips(chips, chain, algo):
    """Samples of the oracle's chips (oracle_ffi CHIP_DTYPE) of one chain and framer that carry the sync flag."""
    sel = (chips["chain"] == chain) & (chips["algo"] == algo) & ((chips["value"] & 2) != 0)
    return chips["sample"][sel].astype(np.int64)
