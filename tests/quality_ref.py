"""Line quality (cfg.line_quality) restated in Python integers: include/wmbus_hip.h, LINE QUALITY, is the definition; this file says the
same on top of repair_ref.py (the walk over the oracle's chips: which telegrams a time2 decoder completes, and where their chips lie) and
level_ref.py (the quantised soft symbol).  Arbitrary precision and floor division: nothing here can overflow or round.  It shares no code
with the kernel.  TEST INFRASTRUCTURE.

    python tests/quality_ref.py        writes tests/golden/quality.json (data only: the records of the bundled capture's lines and of the
                                       first six telegrams of the two synthetic captures of repair_ref.SYNTHETIC)
"""
import json
import os

import numpy as np

import level_ref as LR
import repair_ref as RR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quality.json")
FIELDS = ("n", "chip_rate_chz", "jitter_ns", "hi_hz", "lo_hz", "spread_hz", "eye_hz")
ZERO = dict.fromkeys(FIELDS, 0)
MAX_BYTES = 292                                      # WM_PKT_MAXBYTES
SPAN = 1 << 17                                       # p[n-1] must stay below


def hz(x, n):
    return (3125 * x + 4096 * n) // (8192 * n)


def quality(pos, v, dphi):
    """The record of one subject.  pos: the decimated samples of its n chips from the access-code chip on, v: their values (bit 0
    counts), dphi: the soft-symbol row pos indexes (float32)."""
    pos = [int(x) for x in pos]
    v = [int(x) & 1 for x in v]
    n = len(pos)
    if n < 2:
        return dict(ZERO)
    p = [x - pos[0] for x in pos]
    if p[-1] >= SPAN:
        return dict(ZERO)
    jp = [2 * j - (n - 1) for j in range(n)]
    num = sum(a * b for a, b in zip(jp, p))
    den = n * (n * n - 1) // 3
    assert den == sum(a * a for a in jp)
    n1 = sum(v)
    n0 = n - n1
    if num <= 0 or n1 == 0 or n0 == 0:
        return dict(ZERO)
    assert 80_000_000 * den < 1 << 63
    rate = (80_000_000 * den + num) // (2 * num)
    B = (4 * 65536 * num + den) // (2 * den)
    s = sum(65536 * p[j] - B * j for j in range(n))
    A = (2 * s + n) // (2 * n)
    e = sum(abs(65536 * p[j] - B * j - A) for j in range(n))
    q = [int(x) for x in LR.quantise(np.asarray(dphi, np.float32)[np.asarray(pos, np.int64)])]
    S1 = sum(x for x, b in zip(q, v) if b)
    S0 = sum(x for x, b in zip(q, v) if not b)
    m1, m0 = (2 * S1 + n1) // (2 * n1), (2 * S0 + n0) // (2 * n0)
    mid = (m1 + m0) // 2
    spread = sum(abs(x - (m1 if b else m0)) for x, b in zip(q, v))
    sigma = 1 if m1 >= m0 else -1
    eye = min(sigma * (x - mid) if b else sigma * (mid - x) for x, b in zip(q, v))
    assert rate < 1 << 32
    return dict(n=n, chip_rate_chz=rate, jitter_ns=(1250 * e + 32768 * n) // (65536 * n), hi_hz=hz(m1, 1), lo_hz=hz(m0, 1),
                spread_hz=hz(spread, n), eye_hz=hz(eye, 1))


def quality_telegram(t, dphi):
    """The record of one of repair_ref.telegrams()' telegrams: the n = off + cpb L chips from the access-code chip on."""
    if t["L"] > MAX_BYTES:
        return dict(ZERO)
    n = RR.OFF[t["mode"]] + RR.CPB[t["mode"]] * t["L"]
    assert n <= t["n"]
    return quality(t["pos"][:n], t["v"][:n], dphi)


def quality_capture(ref, push_m=None):
    """One record per line of the oracle's text (oracle_ffi.run with taps, chips and the algorithm tag), in its order.  push_m: decimated
    samples per push (None: one push); a telegram is a subject only if its last chip lies in the push that holds its access code
    (repair_capture's condition), and its positions count from that push's first sample -- which the differences p[j] do not see."""
    done = []
    for chain in (0, 1):
        done += RR.telegrams(ref, chain)
    done.sort(key=lambda t: (t["sample"], t["chain"]))
    out, k = [], 0
    for line in ref["text"].splitlines():
        f = line.split(";")
        if f[0] != "t2a":
            assert f[0] == "rla", "quality_capture needs the oracle's algorithm tag (show_algorithm)"
            out.append(dict(ZERO))
            continue
        t = done[k]; k += 1
        whole = push_m is None or t["pos"][0] // push_m == t["pos"][-1] // push_m
        out.append(quality_telegram(t, ref["dphi_fir"][t["chain"]]) if whole else dict(ZERO))
    assert k == len(done), (k, len(done))
    return out


def make_golden():
    import oracle_ffi as O
    here = os.path.dirname(os.path.abspath(__file__))
    cu8 = np.fromfile(os.path.join(here, "golden", "samples", "rtlsdr_868.950M_1M6_samples2.cu8"), np.uint8)
    cu8 = cu8[:cu8.size // 4096 * 4096]
    ref = O.run(cu8, O.make_opts(), taps=True, chips=True)
    gold = dict(samples2=dict(lines=ref["text"].splitlines(keepends=True), records=quality_capture(ref)), synthetic={})
    for name, (mode, sigma) in RR.SYNTHETIC.items():
        cu8, _ = RR.synthetic(mode, sigma)
        ref = O.run(cu8, O.make_opts(), taps=True, chips=True)
        tg = sorted(RR.telegrams(ref, 0) + RR.telegrams(ref, 1), key=lambda t: (t["sample"], t["chain"]))[:6]
        gold["synthetic"][name] = [quality_telegram(t, ref["dphi_fir"][t["chain"]]) for t in tg]
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    return gold


if __name__ == "__main__":
    print(json.dumps(make_golden(), indent=1))
