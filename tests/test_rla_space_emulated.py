"""The run-length framer over its input space: designed slicer bits (tests/rla_space.py) through the kernel's DEVICE SOURCE on
the host (tests/emu/rla_emu.cpp) against a per-sample restatement of the reference (tests/rla_ref.py) -- chips, the state
record of every segment boundary, and the per-segment access-code flags.  tests/README.md, "The run-length framer's input
space", lists the families, what each is for and what the module costs.  Needs no GPU."""
import collections
import ctypes
import subprocess

import numpy as np
import pytest

import rla_ref
import rla_space as SP
from cases import flags_to_oracle_opts
from test_rla_emulated import emu, interferer_capture, truncate_runs, F_T1C1, F_S1      # noqa: F401 (emu: the fixture)

STATE_DT = np.dtype([(f, "<i4" if f in ("run", "bitlen", "cum", "spb0", "spb1") else "<u4") for f in rla_ref.STATE_FIELDS])
ERR_CHIP_TRUNC = 8


def state_rec(d):
    return np.array([tuple(d[f] for f in rla_ref.STATE_FIELDS)], STATE_DT)[0]


def run_emu(emu, rows, pushes, seg_len, lookback, descending=True, chains=True, cap=None, spill_words=None):
    """The emulated launches of one capture, push by push.  Returns the chips per chain, and per push the converged state
    records [2][nseg] (start, final), the sync_seen flags [2][nseg] and the warning word."""
    assert emu.wm_emu_rla_state_bytes() == STATE_DT.itemsize
    ctypes.c_int.in_dll(emu, "wm_emu_descending").value = int(descending)
    ctypes.c_int.in_dll(emu, "wm_emu_chains").value = int(chains)
    carry = np.zeros(2, STATE_DT)
    for r in range(2):
        emu.wm_emu_rla_reset_state(carry[r:].ctypes.data)
    cap = cap or 8 * seg_len + 8 + 8192
    CH, LV = emu.wm_emu_spill_chunk(), emu.wm_emu_spill_levels()
    out, per_push, m0 = [[], []], [], 0
    try:
        for M in pushes:
            Mcap = (M + 255) // 256 * 256
            words = np.zeros((2, Mcap // 32), np.uint32)
            for ch in range(2):
                b = np.ones(Mcap, np.uint8)                  # what lies beyond the push is not the framer's: ones, so that a missing mask shows
                b[:M] = rows[ch][m0:m0 + M]
                words[ch] = np.packbits(b.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).ravel()
            nseg = (M + seg_len - 1) // seg_len
            chips = np.zeros((2, nseg, cap), np.uint32); counts = np.zeros((2, nseg), np.uint32)
            st0 = np.zeros((2, nseg), STATE_DT); st1 = np.zeros((2, nseg), STATE_DT); seen = np.zeros((2, nseg), np.uint32)
            err = ctypes.c_uint(0)
            if spill_words is not None:
                arena = np.zeros(max(1, spill_words), np.uint32); chain = np.zeros((2, nseg, LV), np.uint32); nchain = np.zeros(2 * nseg + 1, np.uint32)
                emu.wm_emu_rla_set_spill(arena.ctypes.data, spill_words, chain.ctypes.data, nchain.ctypes.data, nchain[2 * nseg:].ctypes.data)
            else:
                emu.wm_emu_rla_set_spill(None, 0, None, None, None)
            ctypes.c_void_p.in_dll(emu, "wm_emu_st_start_out").value = st0.ctypes.data
            ctypes.c_void_p.in_dll(emu, "wm_emu_st_final_out").value = st1.ctypes.data
            ctypes.c_void_p.in_dll(emu, "wm_emu_seen_out").value = seen.ctypes.data
            carried = carry.copy()
            r = emu.wm_emu_rla(words.ctypes.data, 1, M, Mcap, F_T1C1 | F_S1, seg_len, lookback, cap, carry.ctypes.data,
                               chips.ctypes.data, counts.ctypes.data, ctypes.byref(err))
            assert r >= 0, "verification did not converge"
            for ch in range(2):
                for s in range(nseg):
                    n = int(counts[ch, s])
                    w = chips[ch, s, :min(n, cap)]
                    if n > cap:
                        rest = n - cap
                        assert nchain[ch * nseg + s] * CH >= rest
                        w = np.concatenate([w] + [arena[chain[ch, s, l]: chain[ch, s, l] + min(CH, rest - l * CH)] for l in range((rest + CH - 1) // CH)])
                    out[ch].append(np.stack([m0 + s * seg_len + (w >> 3), w & 7], axis=1))
            per_push.append(dict(m0=m0, M=M, start=st0, final=st1, seen=seen, warn=err.value, carried=carried, carry=carry.copy(), reruns=r))
            m0 += M
    finally:
        for name in ("wm_emu_st_start_out", "wm_emu_st_final_out", "wm_emu_seen_out"):
            ctypes.c_void_p.in_dll(emu, name).value = None
    return [np.concatenate(o) if o else np.zeros((0, 2), np.uint32) for o in out], per_push


class Ref:
    """rla_ref over both rows of a stream, once; the states at further samples are computed when a cut asks for them"""
    def __init__(self, rows):
        self.rows, self.res, self.at = rows, None, set()

    def need(self, samples):
        samples = set(samples)
        if self.res is None or not samples <= self.at:
            self.at |= samples
            self.res = [rla_ref.run(ch, self.rows[ch], at=self.at) for ch in (0, 1)]
            self.chips = [r.chips() for r in self.res]
            self.markers = [np.array(sorted(r.marker_samples()), np.int64) for r in self.res]
            self.recs = [{b: state_rec(d).tobytes() for b, d in r.states.items()} for r in self.res]      # WmRlaState records, as bytes
        return self


def boundaries(pushes, seg_len):
    b, m0 = set(), 0
    for P in pushes:
        b.update(range(m0, m0 + P, seg_len)); b.add(m0 + P); m0 += P
    return b


def compare(emu, ref, pushes, seg_len, lookback, what, chips_exact=True, **kw):
    ref.need(boundaries(pushes, seg_len))
    got, per_push = run_emu(emu, ref.rows, pushes, seg_len, lookback, **kw)
    for ch in (0, 1):
        if chips_exact:
            if not np.array_equal(got[ch], ref.chips[ch]):
                n = min(len(got[ch]), len(ref.chips[ch]))
                bad = np.flatnonzero((got[ch][:n] != ref.chips[ch][:n]).any(axis=1))
                i = int(bad[0]) if len(bad) else n
                raise AssertionError(f"{what} chain {ch}: chips differ from chip {i} of {len(got[ch])}/{len(ref.chips[ch])}: "
                                     f"kernel {got[ch][i:i + 3].tolist()} restatement {ref.chips[ch][i:i + 3].tolist()}")
        for p in per_push:
            nseg = p["start"].shape[1]
            for s in range(nseg):
                b0 = p["m0"] + s * seg_len; b1 = min(b0 + seg_len, p["m0"] + p["M"])
                start, final = p["start"][ch, s].tobytes(), p["final"][ch, s].tobytes()
                assert start == (p["final"][ch, s - 1] if s else p["carried"][ch]).tobytes(), (what, ch, b0, "start is not the predecessor's end")
                assert final == ref.recs[ch][b1], (what, ch, f"state behind sample {b1}", dict(zip(rla_ref.STATE_FIELDS, p["final"][ch, s].tolist())), ref.res[ch].states[b1])
                assert start == ref.recs[ch][b0], (what, ch, f"state in front of sample {b0}")
                mk = ref.markers[ch]
                want_seen = bool(np.any((mk >= b0) & (mk < b1)))
                assert bool(p["seen"][ch, s]) == want_seen, (what, ch, f"sync_seen of segment {s} of the push at {p['m0']}", want_seen)
            assert p["carry"][ch].tobytes() == p["final"][ch, nseg - 1].tobytes()
    return got, per_push


def cut(M, sizes=(777, 1029, 2051, 255, 4096, 321, 64, 1, 1283, 6000)):
    """pushes of assorted ragged lengths over M samples"""
    out, i = [], 0
    while M > 0:
        out.append(min(M, sizes[i % len(sizes)])); M -= out[-1]; i += 1
    return out


def three_ways(emu, name, bits, ref=None):
    """as one push; cut into pushes; short segments with every look-back, either lane order, chain walks on and off"""
    rows = bits if isinstance(bits, (list, tuple)) else [bits, bits]
    ref = ref or Ref(rows)
    M = len(rows[0])
    short = cut(M, (5 * 1024 + 3, 11 * 1024, 1024, 7 * 1024 + 1020))
    ref.need(boundaries([M], 1024) | boundaries(cut(M), 8192) | boundaries(short, 1024))      # every state the runs below ask for, in one pass
    compare(emu, ref, [M], 8192, 1024, (name, "one push"))
    compare(emu, ref, cut(M), 8192, 1024, (name, "cut into pushes"))
    for lookback in (32, 64, 256):
        for descending in (True, False):
            for chains in (True, False):
                compare(emu, ref, [M] if lookback != 64 else short, 1024, lookback,
                        (name, f"seg_len 1024 look-back {lookback} descending {descending} chains {chains}"), descending=descending, chains=chains)
    return ref


def positions(events, kinds):
    c = collections.defaultdict(set)
    for e in events:
        if e["kind"] in kinds: c[(e["kind"], e["level"])].add(e["sample"] % 256)
    return c


# ---- the restatement itself, pinned ----------------------------------------------------------------------------------------------
def test_restatement_gives_the_oracles_chips(oracle, samples, wm):
    """rla_ref on the oracle's own slicer bits of the bundled capture and of the interferer capture (bit lengths down to a
    fraction of a sample, three chips per sample): the oracle's run-length chips, chip for chip, reset markers included."""
    for name, cu8 in (("bundled", samples["samples2"]), ("interferer", interferer_capture(wm))):
        o = oracle.run(cu8, flags_to_oracle_opts(oracle, ["-v"]), taps=True, chips=True)
        for ch in (0, 1):
            r = rla_ref.run(ch, o["bit"][ch], rssi=o["rssi"][ch].astype(np.uint32))
            oc = o["chips"][(o["chips"]["chain"] == ch) & (o["chips"]["algo"] == 0)]
            want = np.stack([oc["sample"].astype(np.uint32), oc["value"].astype(np.uint32), oc["rssi"].astype(np.uint32)], axis=1)
            kept = truncate_runs(np.stack([want[:, 0], np.arange(len(want), dtype=np.uint32)], axis=1))[:, 1]      # at most 8192 chips per edge
            assert np.array_equal(r.chips(rssi=True), want[kept]), (name, ch)
            assert len(want) > 5000


def probe_streams():
    """the designed streams that go through the reference itself: all of the small families, a part of the large ones"""
    out = {}
    for ch in (0, 1):
        for fam, streams in (("edge", SP.edge_position(ch)), ("patch", SP.reset_patch(ch)[0]), ("long", SP.long_runs(ch)), ("code", SP.access_code(ch))):
            out.update({f"{fam} {ch} {name}": (ch, bits) for name, bits in streams.items()})
        out[f"staging {ch}"] = (ch, SP.staging(ch))
        out[f"seams {ch}"] = (ch, SP.deglitch_seams()["de Bruijn 11"][:2049 * 12])
    out["half a chip"] = (0, np.concatenate([SP.half_chip_cell(*key) for key in SP.HALF_PATHS]))
    out["settled on 8"] = (0, SP.chip_counts_t1(settle=(8,))["settled on 8"])
    out["spb 13/35"] = (1, SP.chip_counts_s1(pairs=((13, 35),))["spb 13/35"])
    return out


def test_restatement_gives_the_references_own_trace(oracle, tmp_path):
    """The designed streams through the REFERENCE's runlength_algorithm_* (oracle/ref_probe.c, mode `rla`), which writes the
    fields of its state struct behind every sample: rla_ref's trace of the same stream is the same text, line for line (by
    its sha256, recorded with the input's in tests/golden/reference_outputs.json; made anew where oracle/_ref is built).  The
    streams hold access codes but no telegram: the reference prints nothing."""
    for name, (ch, bits) in probe_streams().items():
        raw = np.stack([bits, np.full(len(bits), 40, np.uint8)], axis=1).tobytes()

        def live():
            path = str(tmp_path / "trace.txt")
            out = subprocess.run([oracle.probe_for("rla", tmp_path), "rla", str(ch), path], input=raw, capture_output=True, check=True).stdout
            with open(path, "rb") as f:
                return {"input": oracle.sha256(raw), "trace": oracle.sha256(f.read()), "stdout": oracle.sha256(oracle.mask_ts(out))}
        want = oracle.reference_answer(f"ref_probe rla {name}", live)
        assert want["input"] == oracle.sha256(raw), (name, "the stream is not the one the reference's answer was recorded for")
        assert want["stdout"] == oracle.sha256(b""), name
        lines = []
        rla_ref.run(ch, bits, trace=lines)
        assert len(lines) == len(bits) and oracle.sha256("".join(lines).encode()) == want["trace"], name


# ---- the families ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, 1])
def test_edge_at_every_sample_of_a_step(emu, chain):
    """Every kind of edge of the chain -- a chip run and each of its reset rules -- ending a run of either level at every
    sample of a 256-sample step: w 0..3 x k 0..63, so k = 0 behind a word and a step boundary and k = 63 among them; the
    three ways put them behind segment and push boundaries too."""
    seen = collections.defaultdict(set)
    for name, bits in SP.edge_position(chain).items():
        ref = three_ways(emu, ("edge position", chain, name), bits)
        for key, pos in positions(ref.res[chain].events, rla_ref.KINDS[chain]).items():
            seen[key] |= pos
    for kind in rla_ref.KINDS[chain]:
        for level in (0, 1):
            assert seen[(kind, level)] == set(range(256)), (chain, kind, level, sorted(set(range(256)) - seen[(kind, level)]))


@pytest.mark.parametrize("chain", [0, 1])
def test_reset_patch_across_word_step_segment_and_push(emu, chain):
    """A reset at k = 58..63 of each word of a step; the five raw samples behind it take all 32 values, so the five patched
    levels cross into the next word and step (and, cut as below, the next segment and push), and for many of the values a
    second reset falls inside those five samples."""
    streams, resets = SP.reset_patch(chain)
    bits = streams["patch"]
    ref = three_ways(emu, ("reset patch", chain), bits)
    at = {e["sample"]: e for e in ref.res[chain].events}
    second = collections.Counter()
    for p in resets:
        assert p in at and at[p]["kind"] != rla_ref.CHIPS, (chain, p)
        second[(p % 64, p // 64 % 4)] += any(p + j in at and at[p + j]["kind"] != rla_ref.CHIPS for j in range(1, 6))
    assert {(k, w) for k in range(58, 64) for w in range(4)} == set(second) and min(second.values()) >= 4, second
    # pushes and 1024-sample segments that end right behind each reset, so that the patch is the carried state's business
    for off in (1, 2, 3, 6):
        cuts = sorted(set(p + off for p in resets[::7]))
        pushes = [b - a for a, b in zip([0] + cuts, cuts + [len(bits)]) if b > a]
        compare(emu, ref, pushes, 1024, 32, ("reset patch", chain, f"pushes end {off} behind a reset"))


def test_every_raw_window_across_half_word_word_and_step(emu):
    """Every 11-bit raw window (so every 8-bit one: the index space of lut[] and of both halves of deglitch64) at every sample
    of a step, hence at every alignment across a half-word, a word and a step boundary."""
    bits = SP.deglitch_seams()["de Bruijn 11"]
    w = np.zeros(len(bits) - 10, np.int64)
    for j in range(11):
        w |= bits[j:len(bits) - 10 + j].astype(np.int64) << j
    seen = np.zeros((2048, 256), bool)
    seen[w, np.arange(len(w)) % 256] = True
    assert seen.all()
    ref = three_ways(emu, "deglitcher seams", bits)
    assert len(ref.res[0].events) > 50000 and len(ref.res[1].events) > 50000


def test_chip_counts_t1c1(emu):
    """The tracker settled on chips of 6..12 samples, then every run of 5..400 samples; and a run of exactly half a chip
    (reset) and of half a chip and 1/256 sample (one chip) at bit lengths 2 * 256 r (+ 1, - 1, - 2), r = 5..8, either level."""
    for name, bits in SP.chip_counts_t1().items():
        c = int(name.split()[-1])
        ref = three_ways(emu, ("chip counts", name), bits)
        ev = ref.res[0].events
        got = {b["run"] for a, b in zip(ev, ev[1:]) if a["run"] == c and a["kind"] == rla_ref.CHIPS}
        assert got >= set(range(5, 401)), (name, sorted(set(range(5, 401)) - got))
    cells = {key: SP.half_chip_cell(*key) for key in SP.HALF_PATHS}
    ref = three_ways(emu, "half a chip", np.concatenate(list(cells.values())))
    hits = {(e["unit"], e["level"]): e for e in ref.res[0].events if e["run"] == (e["unit"] + 2) // 512}
    for (bitlen, level) in cells:
        e = hits[(bitlen, level)]
        r = (bitlen + 2) // 512
        if bitlen % 512 < 2:
            assert e["kind"] == rla_ref.RST_HALF and 256 * r == e["half"]
        else:
            assert e["kind"] == rla_ref.CHIPS and e["n"] == 1 and 256 * r == e["half"] + 1


def test_chip_counts_s1(emu):
    """The two samples-per-bit trackers at pairs across 13..35, then every run of 1..300 samples at either level (S1 has no
    high run of 2 or 3 samples); their mean at 12, 13, 35 and 36; a run of exactly half a bit and of one sample more."""
    seen_units = set()
    for name, bits in SP.chip_counts_s1().items():
        a, b = map(int, name.split()[1].split("/"))
        ref = three_ways(emu, ("chip counts", name), bits)
        got = {0: set(), 1: set()}
        for e in ref.res[1].events:
            if e["unit"] == (a + b) // 2 and e["kind"] != rla_ref.RST_SPB: got[e["level"]].add(e["run"])
            seen_units.add(e["unit"])
        assert got[0] >= set(range(1, 301)) and got[1] >= {1} | set(range(4, 301)), (name, sorted(set(range(1, 301)) - got[0]), sorted(set(range(4, 301)) - got[1]))
        half = (a + b) // 2 // 2
        kinds = {e["run"]: e["kind"] for e in ref.res[1].events if e["unit"] == (a + b) // 2 and e["run"] in (half, half + 1)}
        assert kinds == {half: rla_ref.RST_RUN0, half + 1: rla_ref.CHIPS}, (name, kinds)
    assert len(SP.chip_counts_s1()) == len(SP.S1_PAIRS)                      # every pair can be reached from reset
    edge = SP.edge_position(1)
    for name in ("spb low side", "spb high side"):
        seen_units |= {e["unit"] for e in rla_ref.run(1, edge[name][:6000]).events}
    assert {12, 13, 35, 36} <= seen_units


@pytest.mark.parametrize("chain", [0, 1])
def test_long_runs_then_the_access_code(emu, chain):
    """n = 23..26 chips (the shift register takes at most 24 more at once), 32 n around 4096, 8191..8193 chips (the chip
    limit), runs of 65524..65545 samples (T1/C1: the first division's dividend crosses 2^24) -- each followed at once by the
    chain's access code, whose marker must come out behind the collapsed shift, a long low run being the code's first chip."""
    ns, ua, b2, marks, cells = set(), [], set(), 0, 0
    for name, bits in SP.long_runs(chain).items():
        ref = three_ways(emu, ("long runs", chain, name), bits)
        for e in ref.res[chain].events:
            if e["kind"] == rla_ref.CHIPS:
                ns.add(e["n"]); ua.append(e["div"][0][0]); b2.add(e["div"][1][1])
        marks += len(ref.res[chain].marker_samples())
    want_cells = (2 * len(SP.LONG_T1[0]) + len(SP.LONG_T1[1]) + len(SP.LONG_T1[2])) if chain == 0 else 2 * len(SP.LONG_S1[0]) + len(SP.LONG_S1[1])
    assert marks == want_cells                                                 # every code behind every long run is found
    assert ns >= {23, 24, 25, 26, 8191, 8192, 8193}
    if chain == 0:
        assert ns >= {127, 128, 129} and {32 * 127, 32 * 128} <= b2
        assert min(u for u in ua if u > 1 << 23) < 1 << 24 <= max(ua) and (1 << 24) - 1 in ua      # both sides of wm_udiv's dividend bound, and the last value below it


@pytest.mark.parametrize("chain", [0, 1])
def test_access_code_placements(emu, chain):
    """The marker chip at every k of a word; the code directly behind a reset; every single-chip near miss (no marker); two
    codes back to back."""
    streams = SP.access_code(chain)
    refs = {name: three_ways(emu, ("access code", chain, name), bits) for name, bits in streams.items()}
    mk = {name: r.res[chain].marker_samples() for name, r in refs.items()}
    assert {m % 64 for m in mk["marker at every k"]} == set(range(64)) and len(mk["marker at every k"]) == 64
    assert len(mk["behind a reset"]) == 2 and len(mk["back to back"]) == 2 and mk["near misses"] == []
    first = [v for (_, v, _, _, _) in refs["behind a reset"].res[chain].runs if v & 4]
    assert len(first) >= 2                                                     # the code's first chip carries the reset marker


def test_ragged_pushes(emu):
    """Pushes ending at every residue of a step (so 1..63 of a word), runs of pushes that each end 1..4 samples into a word
    (the carried raw history is then older than the push), and pushes of 1..5 samples.  Emulator only: the product's pushes
    are multiples of 2048 input samples, which reach the residues 1..4 (tests/test_gpu_rla_space.py) and few others."""
    base = SP.ragged_base()
    a, b, c = SP.ragged_pushes()
    rows = [base, base[::-1].copy()]
    for name, pushes in (("every residue", a), ("1..4 into a word", b + c + b), ("tiny", c + c + [700] + c)):
        assert sum(pushes) <= len(base)
        ref = Ref([r[:sum(pushes)] for r in rows])
        for lookback in (32, 256):
            compare(emu, ref, pushes, 1024, lookback, ("ragged", name, lookback))
    assert {p % 256 for p in a} == set(range(1, 256)) and {p % 64 for p in b} == {1, 2, 3, 4} and set(c) == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("chain", [0, 1])
def test_staging_and_storage_around_a_small_primary_region(emu, chain):
    """cap small, a multiple of 8: the segments' chip counts take every value in cap - 8 .. cap + 8, so every residue mod 8
    of the staged groups on either side of the region's end.  With a roomy spill arena the chips are the restatement's; with
    an arena of exactly one chunk, or none, WM_ERR_CHIP_TRUNC is raised, every state record is still exact and what was kept
    of each segment is a prefix of its chips."""
    bits, cap = SP.staging(chain), SP.STAGING_CAP[chain]
    M = len(bits)
    ref = Ref([bits, bits]).need(boundaries([M], 1024))
    counts = np.bincount(ref.chips[chain][:, 0] // 1024, minlength=M // 1024)
    assert set(range(cap - 8, cap + 9)) <= set(counts.tolist())
    other = np.bincount(ref.chips[1 - chain][:, 0] // 1024, minlength=M // 1024)
    for pushes in ([M], cut(M, (7 * 1024, 1024, 12 * 1024))):         # whole segments, so that a chip's position names its segment
        for lookback in (32, 256):
            got, per_push = compare(emu, ref, pushes, 1024, lookback, ("staging", chain, "arena"), cap=cap, spill_words=1 << 20)
            assert all(p["warn"] == 0 for p in per_push)
            for words in (emu.wm_emu_spill_chunk(), None):
                got, per_push = compare(emu, ref, pushes, 1024, lookback, ("staging", chain, words), chips_exact=False, cap=cap, spill_words=words)
                assert any(p["warn"] == ERR_CHIP_TRUNC for p in per_push) and all(p["warn"] in (0, ERR_CHIP_TRUNC) for p in per_push)
                for ch in (0, 1):
                    lost = 0
                    seg_g, seg_w = got[ch][:, 0] // 1024, ref.chips[ch][:, 0] // 1024
                    for sg in range(M // 1024):
                        g, w = got[ch][seg_g == sg], ref.chips[ch][seg_w == sg]
                        assert len(g) <= len(w) and np.array_equal(g, w[:len(g)]), (chain, ch, sg, words)
                        assert len(g) == len(w) or len(g) >= cap - 7              # nothing is lost below the primary region
                        lost += len(w) - len(g)
                    assert (lost > 0) == bool((counts if ch == chain else other).max() > cap), (chain, ch, words, lost)


def test_division_operands_reach_every_branch_of_wm_udiv():
    """What the families feed the kernel's three divisions (chips per run; the bit-length update; S1 samples per bit), read
    from the restatement's events: a divisor on either side of 4 and of 4096, a dividend on either side of 2^24, exact
    multiples of the divisor, and negative dividends through wm_sdiv.  (Divisors below 4 in the FIRST division -- a bit
    length dragged to nothing -- stay the interferer capture's case, tests/test_rla_emulated.py.)"""
    ops = []
    for chain, streams in ((0, SP.long_runs(0)), (1, SP.long_runs(1)), (1, {"s": SP.chip_counts_s1(pairs=((24, 24),))["spb 24/24"]}),
                           (0, {"c": SP.chip_counts_t1(settle=(8,))["settled on 8"]})):
        for bits in streams.values():
            for e in rla_ref.run(chain, bits).events:
                ops += list(e["div"])
    b = {d for _, d in ops}; a = [n for n, _ in ops]
    assert {1, 2, 3, 4, 5} <= b                                                # S1 run0 / n: the integer divide below 4, the reciprocal from 4
    assert {32 * 127, 32 * 128} <= b and max(b) >= 32 * 8193                   # the bit-length update at and beyond 4096
    assert (1 << 24) - 1 in a and max(a) >= 1 << 24                            # the dividend bound
    assert min(a) < 0                                                          # wm_sdiv's sign handling
    assert any(n > 0 and n % d == 0 and 4 <= d < 4096 for n, d in ops) and any(n % d == d - 1 and 4 <= d < 4096 for n, d in ops if n > 0)
