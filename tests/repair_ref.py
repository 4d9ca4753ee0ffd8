"""CRC repair (cfg.crc_repair) restated in numpy and Python integers: include/wmbus_hip.h, CRC REPAIR, is the definition; this file says
the same on top of telegram_ref.py (framing, what a decoder does with the chips behind an access code) and level_ref.py (the quantised
soft symbol and the preamble window).  It shares no code with the kernel.  TEST INFRASTRUCTURE.

    python tests/repair_ref.py        writes tests/golden/repair.json (data only: the expected text and the counts of the three captures)
"""
import json
import os

import numpy as np

import level_ref as LR
import telegram_ref as TR

K = 8                                                # candidates per bad block
CPB = {"T1": 12, "C1": 8, "S1": 16}                  # chips per byte
OFF = {"T1": 1, "C1": 17, "S1": 1}                   # chip of byte 0's first chip; j = 0 is the access-code chip
ALGO_T2A = 1
NIBBLE = np.full(64, 255, np.int64)
for _s, _n in TR.NIBBLE_OF_SYMBOL.items():
    NIBBLE[_s] = _n
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repair.json")
ZERO = dict(blocks_bad=0, blocks_repaired=0, chips_flipped=0, weight=0)


def preamble_mean(dphi, a, chain):
    """c: LINE LEVELS' mean over the preamble window in front of access-code sample a, 0 where that record is invalid (n = 0)."""
    lo, hi = LR.LO[chain], LR.HI[chain]
    if a - lo < 0:
        return 0
    n = lo - hi
    total = sum(int(x) for x in LR.quantise(dphi[a - lo:a - hi]))
    return (2 * total + n) // (2 * n)


def reliabilities(dphi, pos, c):
    """r[j] = |q[j] - c| for the chips at decimated samples pos."""
    return np.abs(LR.quantise(np.asarray(dphi, np.float32)[np.asarray(pos, np.int64)]) - int(c))


def decode_rows(mode, C):
    """C [P, n x cpb] chip bits -> (bytes [P, n] int64, valid [P]): every row decoded by the mode's line code; a row is valid if every
    3-out-of-6 symbol (T1) or Manchester pair (S1) in it is a code word (C1: always).  An invalid T1 symbol reads as 0xFF."""
    C = np.asarray(C, np.int64)
    P = C.shape[0]
    if mode == "C1":
        b = C.reshape(P, -1, 8)
        return (b << np.arange(7, -1, -1)).sum(axis=2), np.ones(P, bool)
    if mode == "T1":
        sym = (C.reshape(P, -1, 2, 6) << np.arange(5, -1, -1)).sum(axis=3)
        nib = NIBBLE[sym]
        bad = (nib == 255).any(axis=2)
        return np.where(bad, 255, nib[:, :, 0] << 4 | nib[:, :, 1] & 15), ~bad.any(axis=1)
    pair = C.reshape(P, -1, 8, 2)
    pair = pair[..., 0] * 2 + pair[..., 1]
    return ((pair == 1).astype(np.int64) << np.arange(7, -1, -1)).sum(axis=2), ((pair == 1) | (pair == 2)).all(axis=(1, 2))


def crc16_rows(B):
    """EN 13757 CRC-16 of every row of B [P, n]."""
    crc = np.zeros(B.shape[0], np.int64)
    for k in range(B.shape[1]):
        crc ^= B[:, k] << 8
        for _ in range(8):
            crc = np.where(crc & 0x8000, (crc << 1) ^ 0x3D65, crc << 1) & 0xFFFF
    return crc ^ 0xFFFF


def repair_block(mode, cb, rb, excluded):
    """The repair of one bad block: cb its chips, rb their reliabilities, `excluded` leading chips that are no candidates (the L-field
    byte's).  None, or (m, w, [flipped chip indices within the block])."""
    cpb = CPB[mode]
    if len(cb) // cpb < 3:
        return None
    cand = sorted(range(excluded, len(cb)), key=lambda j: (int(rb[j]), j))[:K]
    m = np.arange(1, 1 << len(cand), dtype=np.int64)
    C = np.tile(np.asarray(cb, np.int64) & 1, (m.size, 1))
    w = np.zeros(m.size, np.int64)
    for i, j in enumerate(cand):
        on = (m >> i) & 1 == 1
        C[on, j] ^= 1
        w[on] += int(rb[j])
    B, valid = decode_rows(mode, C)
    ok = valid & (crc16_rows(B[:, :-2]) == (B[:, -2] << 8 | B[:, -1]))
    if not ok.any():
        return None
    best = min((int(w[i]), int(m[i])) for i in np.nonzero(ok)[0])
    return best[1], best[0], [j for i, j in enumerate(cand) if best[1] >> i & 1]


def repair_telegram(mode, frame_b, L, v, r):
    """A subject's verdict.  v: chip bits from the access-code chip on (index j), r: their reliabilities, L: air bytes.
    dict(record, repaired, air, err3of6): air and err3of6 are the repaired telegram's where repaired, else None."""
    off, cpb = OFF[mode], CPB[mode]
    v = np.asarray(v, np.int64).copy() & 1
    air, _ = decode_rows(mode, v[None, off:off + cpb * L])
    air = bytes(air[0].tolist())
    rec = dict(ZERO)
    for start, blk in TR.blocks(frame_b, L):
        if blk >= 2 and TR.crc16(air[start:start + blk - 2]) == (air[start + blk - 2] << 8 | air[start + blk - 1]):
            continue
        rec["blocks_bad"] += 1
        j0, j1 = off + cpb * start, off + cpb * (start + blk)
        res = repair_block(mode, v[j0:j1], r[j0:j1], cpb if start == 0 else 0)
        if res is None:
            continue
        rec["blocks_repaired"] += 1
        rec["chips_flipped"] += len(res[2])
        rec["weight"] += res[1]
        for j in res[2]:
            v[j0 + j] ^= 1
    if rec["blocks_repaired"] != rec["blocks_bad"]:
        return dict(record=rec, repaired=False, air=None, err3of6=None)
    fixed, valid = decode_rows(mode, v[None, off:off + cpb * L])
    fixed = bytes(fixed[0].tolist())
    assert TR.crc_clean(frame_b, fixed, L)
    return dict(record=rec, repaired=True, air=fixed, err3of6=mode == "T1" and not bool(valid[0]))


def format_line(mode, crc_ok, err3of6, pkt_rssi, rssi_now, frame_b, air, L, tag="t2a;"):
    """A datagram line with the fixed timestamp, as the decoders print it."""
    pkt = bytes(air) + bytes(8)
    ident = pkt[4] | pkt[5] << 8 | pkt[6] << 16 | pkt[7] << 24
    ok3 = 1 if mode == "S1" else int(not err3of6)
    return f"{tag}{mode};{int(crc_ok)};{ok3};TS;{pkt_rssi};{rssi_now};{ident:08X};0x{TR.printed_hex(frame_b, air, L)}\n"


def telegrams(ref, chain, dphi=None):
    """Every telegram the time2 decoder of `chain` completes on the oracle's chips, in chip order: what a decoder does from each
    access-code chip it is idle for (telegram_ref.expect).  dicts of i (index of the access-code chip in the chain's chip stream), n
    (chips consumed), pos (their samples), v (their bits), mode, and expect's fields."""
    oc = ref["chips"][(ref["chips"]["chain"] == chain) & (ref["chips"]["algo"] == ALGO_T2A)]
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
        n = e["consumed"]
        if e["done"]:
            mode = "S1" if chain else "C1" if e["c1"] else "T1"
            out.append(dict(e, i=i, n=n, pos=pos[i:i + n], v=val[i:i + n] & 1, mode=mode, chain=chain, sample=int(pos[i + n - 1])))
        i += n
    return out


def repair_capture(ref, push_m=None):
    """The lines, crc_ok flags and repair records a context with crc_repair = 1 gives for a capture, from the oracle's run of it
    (oracle_ffi.run with taps, chips and the algorithm tag).  push_m: decimated samples per push (None: one push); a telegram is a
    subject only if its last chip lies in the push that holds its access code.  Returns dict(lines=[text], crc_ok=[0 / 1],
    records=[dict], repaired=[bool], subjects=n, sent=[air bytes of every repaired line])."""
    done = []
    for chain in (0, 1):
        for t in telegrams(ref, chain):
            done.append(t)
    done.sort(key=lambda t: (t["sample"], t["chain"]))
    lines = ref["text"].splitlines(keepends=True)
    out = dict(lines=[], crc_ok=[], records=[], repaired=[], subjects=0, air=[])
    k = 0
    for line in lines:
        f = line.split(";")
        if f[0] != "t2a":
            assert f[0] == "rla", "repair_capture needs the oracle's algorithm tag (show_algorithm)"
            out["lines"].append(line); out["crc_ok"].append(int(f[2])); out["records"].append(dict(ZERO)); out["repaired"].append(False); out["air"].append(None)
            continue
        t = done[k]; k += 1
        L, fb = t["L"], t["frame_b"]
        air = t["bytes"][:L]
        mine = format_line(t["mode"], t["crc_ok"], t["err3of6"], t["pkt_rssi"], t["rssi_now"], fb, t["bytes"][:max(L, 2)], L)
        assert mine == line, (mine, line)                # the walk over the chips is the oracle's decoder
        rec, repaired = dict(ZERO), False
        whole = push_m is None or t["pos"][0] // push_m == t["pos"][-1] // push_m
        if whole and not t["crc_ok"] and L >= 12:
            out["subjects"] += 1
            a = int(t["pos"][0])
            dphi = ref["dphi_fir"][t["chain"]]
            res = repair_telegram(t["mode"], fb, L, t["v"], reliabilities(dphi, t["pos"], preamble_mean(dphi, a, t["chain"])))
            rec, repaired = res["record"], res["repaired"]
            if repaired:
                air = res["air"]
                line = format_line(t["mode"], 1, res["err3of6"], t["pkt_rssi"], t["rssi_now"], fb, air, L)
        out["lines"].append(line); out["crc_ok"].append(1 if repaired else int(f[2])); out["records"].append(rec); out["repaired"].append(repaired)
        out["air"].append(air)
    assert k == len(done), (k, len(done))
    return out


# ---- the three captures the defaults rest on -------------------------------------------------------------------------------------
def synthetic(mode, sigma):
    """(cu8, sent air bytes): 60 frame A telegrams of L-field 40 from default_rng(5), modulated at amplitude 40 over noise `sigma`."""
    rng = np.random.default_rng(5)
    sent = []
    for _ in range(60):
        t = rng.integers(0, 256, 41).astype(np.uint8)
        t[0] = 40
        sent.append(TR.frame_a(bytes(t)))
    return TR.modulate([(mode, a) for a in sent], seed=3, amplitude=40, sigma=sigma), sent


SYNTHETIC = {"t1-sigma32": ("T1", 32), "c1a-sigma30": ("C1A", 30)}


def counts(res, sent):
    """Of the telegrams that reach the time2 decoder with the right L-field: clean, repaired, still bad; and the false repairs."""
    want = TR.frame_a_length(40)
    n = dict(reached=0, clean=0, repaired=0, bad=0, false_repairs=0)
    for line, air, rep in zip(res["lines"], res["air"], res["repaired"]):
        if not line.startswith("t2a;") or air is None or len(air) != want:
            continue
        n["reached"] += 1
        if rep:
            n["repaired"] += 1
            n["false_repairs"] += bytes(air) not in sent
        elif line.split(";")[2] == "1":
            n["clean"] += 1
        else:
            n["bad"] += 1
    return n


def make_golden():
    import oracle_ffi as O
    here = os.path.dirname(os.path.abspath(__file__))
    cu8 = np.fromfile(os.path.join(here, "golden", "samples", "rtlsdr_868.950M_1M6_samples2.cu8"), np.uint8)
    cu8 = cu8[:cu8.size // 4096 * 4096]
    res = repair_capture(O.run(cu8, O.make_opts(), taps=True, chips=True))
    gold = dict(samples2=dict(lines=res["lines"], crc_ok=res["crc_ok"], records=res["records"], subjects=res["subjects"]), synthetic={})
    for name, (mode, sigma) in SYNTHETIC.items():
        cu8, sent = synthetic(mode, sigma)
        gold["synthetic"][name] = counts(repair_capture(O.run(cu8, O.make_opts(), taps=True, chips=True)), sent)
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")
    return gold


if __name__ == "__main__":
    print(json.dumps(make_golden(), indent=1))
