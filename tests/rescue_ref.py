"""S1 rescue (cfg.s1_rescue) restated in numpy and Python integers: include/wmbus_hip.h, S1 RESCUE, is the definition; this file says the
same on top of telegram_ref.py (framing, what a decoder does with the chips behind an access code), level_ref.py (the quantised soft
symbol) and the chip walk of repair_ref.telegrams, extended to both framers and to the aborts.  It shares no code with the kernel.
TEST INFRASTRUCTURE.

    python tests/rescue_ref.py        writes tests/golden/rescue.json (data only: the counts of the two synthetic captures)
"""
import json
import os

import numpy as np

import level_ref as LR
import repair_ref as RR
import telegram_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rescue.json")
ZERO = dict(status=0, pairs=0, min_margin=0, blocks=0)
MAX_BYTES = 292                                      # WM_PKT_MAXBYTES
CHAIN_S1, ALGO_T2A = 1, 1


def decide(v, q):
    """The decision over the data chips v (chip 1 on, an even number) with the quantised soft symbols q at their samples:
    (bits, number of invalid pairs, their smallest margin or None).  A valid pair keeps its hard value (01 -> 1, 10 -> 0); of an
    invalid one the chip with the larger soft symbol is the 1, a tie reads 0."""
    bits, margins = [], []
    for k in range(len(v) // 2):
        a, b = int(v[2 * k]) & 1, int(v[2 * k + 1]) & 1
        if a != b:
            bits.append(b)
        else:
            qa, qb = int(q[2 * k]), int(q[2 * k + 1])
            bits.append(1 if qb > qa else 0)
            margins.append(abs(qb - qa))
    return bits, len(margins), (min(margins) if margins else None)


def n_blocks(L):
    return len(TR.blocks(False, L))


def rescue_telegram(L, v, q):
    """A subject's verdict.  v: the 16 L data chips, q: their quantised soft symbols.  dict(record, rescued, air)."""
    bits, pairs, margin = decide(v[:16 * L], q[:16 * L])
    air = bytes(int("".join(map(str, bits[8 * b:8 * b + 8])), 2) for b in range(L))
    clean = TR.crc_clean(False, air, L)
    return dict(record=dict(status=1 if clean else 2, pairs=pairs, min_margin=margin, blocks=n_blocks(L)), rescued=clean, air=air if clean else None)


def examine(val, rssi, consumed):
    """What the rule makes of an abort of the S1 chain's time2 decoder that has all the chips it asks about: val / rssi the chip
    values (bit 0 the chip, bit 2 the framer-reset marker) and RSSI bytes from the access-code chip on, `consumed` what the decoder
    took.  (kind, L): kind "no" -- nothing the rule looks at (no length, or not a Manchester abort); "short" -- the stream ends before
    chip n - 1; "gated" -- a Manchester abort that a reset marker or the RSSI gate would have stopped anyway; "subject"."""
    val = np.asarray(val, np.int64)
    v = val & 1
    if len(v) < 17:
        return "no", 0
    pairs = v[1:17:2] * 2 + v[2:17:2]
    if ((pairs == 0) | (pairs == 3)).any():
        return "no", 0                                   # an invalid pair inside the L-field: the length is not known
    L = TR.frame_a_length(int("".join("1" if p == 1 else "0" for p in pairs), 2))
    if L < 12 or L > MAX_BYTES:
        return "no", L
    n = 1 + 16 * L
    if len(v) < n:
        return "short", L
    pair = v[1:n:2] * 2 + v[2:n:2]
    bad = np.nonzero((pair == 0) | (pair == 3))[0]
    if bad.size == 0 or consumed != 2 * int(bad[0]) + 3:
        return "no", L
    if (val[1:n] & 4).any() or (np.asarray(rssi, np.int64)[1:n - 1] < TR.RSSI_GATE).any():
        return "gated", L
    return "subject", L


def walk(ref, chain, algo):
    """What the decoder of (chain, framer) does on the oracle's chips, access code by access code it is idle for (telegram_ref.expect),
    in chip order: dicts of i (index of the access-code chip in the chip stream), consumed, done, and expect's fields; plus the
    stream's arrays (val, rssi, pos)."""
    oc = ref["chips"][(ref["chips"]["chain"] == chain) & (ref["chips"]["algo"] == algo)]
    val, rssi, pos = oc["value"].astype(np.int64), oc["rssi"].astype(np.int64), oc["sample"].astype(np.int64)
    longest = 16 * TR.MAX_AIR + 2
    out, i = [], 0
    sync = np.nonzero(val & 2)[0]
    while True:
        k = np.searchsorted(sync, i)
        if k == sync.size:
            break
        i = int(sync[k])
        w = val[i:i + longest]
        e = TR.expect("S1" if chain else "T1", w, rssi[i:i + longest], resets=np.nonzero(w & 4)[0].tolist())
        if e is None:
            break                                        # the stream ends inside the burst
        out.append(dict(e, i=i))
        i += e["consumed"]
    return out, val, rssi, pos


def rescue_capture(ref, push_m=None):
    """The lines, crc_ok flags, rescue records and stats a context with s1_rescue = 1 gives for a capture, from the oracle's run of it
    (oracle_ffi.run with taps, chips and the algorithm tag).  push_m: decimated samples per push (None: one push); an abort is
    examined only if all its n chips lie in the push that holds its access code.  Returns dict(lines=[text], crc_ok=[0 / 1],
    records=[dict], rescued=[bool], air=[bytes of a rescued line or None], stats=(subjects, rescued), gated=n, bad=[record of every
    subject with a bad block], plain=[index into the oracle's lines, or None for a rescued line])."""
    rows = []                                            # (sample, chain, algo, seq, line, crc_ok, record, air)
    stats, gated, bad = [0, 0], 0, []
    for chain in (0, 1):
        for algo in (0, 1):
            events, val, rssi, pos = walk(ref, chain, algo)
            seq = 0
            for e in events:
                i, n = e["i"], e["consumed"]
                if e["done"]:
                    mode = "S1" if chain else "C1" if e["c1"] else "T1"
                    L = e["L"]
                    line = RR.format_line(mode, e["crc_ok"], e["err3of6"], e["pkt_rssi"], e["rssi_now"], e["frame_b"], e["bytes"][:max(L, 2)], L,
                                          tag="t2a;" if algo else "rla;")
                    rows.append((int(pos[i + n - 1]), chain, algo, seq, line, int(e["crc_ok"]), dict(ZERO), None)); seq += 1
                    continue
                if chain != CHAIN_S1 or algo != ALGO_T2A:
                    continue
                kind, L = examine(val[i:i + 1 + 16 * MAX_BYTES], rssi[i:i + 1 + 16 * MAX_BYTES], n)
                if kind in ("no", "short"):
                    continue
                m = 1 + 16 * L
                if push_m is not None and pos[i] // push_m != pos[i + m - 1] // push_m:
                    continue
                if kind == "gated":
                    gated += 1
                    continue
                q = LR.quantise(np.asarray(ref["dphi_fir"][chain], np.float32)[pos[i + 1:i + m]])
                res = rescue_telegram(L, val[i + 1:i + m] & 1, q)
                stats[0] += 1
                if not res["rescued"]:
                    bad.append(res["record"])
                    continue
                stats[1] += 1
                line = RR.format_line("S1", 1, False, int(rssi[i + 1]), int(rssi[i + m - 1]), False, res["air"], L)
                rows.append((int(pos[i + m - 1]), chain, algo, seq, line, 1, res["record"], res["air"])); seq += 1
    rows.sort(key=lambda r: r[:4])
    plain = ref["text"].splitlines(keepends=True)
    mine = [r[4] for r in rows if r[7] is None]
    assert mine == plain, (len(mine), len(plain))          # the walk over the chips is the oracle's decoders, both framers
    out = dict(lines=[r[4] for r in rows], crc_ok=[r[5] for r in rows], records=[r[6] for r in rows], rescued=[r[7] is not None for r in rows],
               air=[r[7] for r in rows], stats=tuple(stats), gated=gated, bad=bad, plain=[])
    k = 0
    for r in rows:
        out["plain"].append(None if r[7] is not None else k)
        k += r[7] is None
    return out


# ---- the two captures the rule rests on ---------------------------------------------------------------------------------------------
SYNTHETIC = {"s1-l40": ([40] * 12, 30), "s1-mixed": ([9, 25, 26, 255] * 3, 30)}      # name: (L-fields, noise sigma)


def synthetic(name):
    """(cu8, sent air bytes): frame A telegrams of the capture's L-fields from default_rng(5) as in repair_ref.synthetic, S1, modulated at
    amplitude 40 over the capture's noise sigma, seed 3."""
    lfields, sigma = SYNTHETIC[name]
    rng = np.random.default_rng(5)
    sent = []
    for lf in lfields:
        t = rng.integers(0, 256, lf + 1).astype(np.uint8)
        t[0] = lf
        sent.append(TR.frame_a(bytes(t)))
    return TR.modulate([("S1", a) for a in sent], seed=3, amplitude=40, sigma=sigma), sent


def counts(res, sent):
    """Per capture: the telegrams sent, the S1 telegrams the oracle's time2 decoder prints CRC-clean anyway, the subjects, the rescued,
    the subjects with a bad block, the Manchester aborts the RSSI gate or a reset leaves out, the false rescues."""
    clean = sum(1 for line, rec in zip(res["lines"], res["rescued"]) if not rec and line.startswith("t2a;S1;1;"))
    return dict(sent=len(sent), decoded=clean, subjects=res["stats"][0], rescued=res["stats"][1], bad=len(res["bad"]), gated=res["gated"],
                false_rescues=sum(1 for a in res["air"] if a is not None and bytes(a) not in sent))


def make_golden():
    import oracle_ffi as O
    gold = {}
    for name in SYNTHETIC:
        cu8, sent = synthetic(name)
        gold[name] = counts(rescue_capture(O.run(cu8, O.make_opts(), taps=True, chips=True)), sent)
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    return gold


if __name__ == "__main__":
    print(json.dumps(make_golden(), indent=1))
