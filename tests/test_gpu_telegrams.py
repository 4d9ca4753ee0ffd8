"""The compiled burst kernels over the telegram space, through the C ABI: captures modulated by tests/telegram_ref.py (one per mode,
L-fields at the edges of the frame formats and on either side of 64, 128, 192 and 256 air bytes -- the byte loop of k3_bursts works in
trips of 64 lanes) decoded in one push (the kernel decodes every telegram), with every burst sent to the host decoders, in small pushes
that cut every telegram, in 1024-sample segments in both clock forms, with and without the debug taps, and three modes side by side in
one context.  The expectation is the oracle's text on the same bytes, byte for byte; a CPU test states what that text must hold -- a
run-length and a time2 line for EVERY telegram, with the restated hex and CRC verdict -- so that no GPU test passes on an empty text."""
import numpy as np
import pytest

import telegram_ref as TR

FS = 1.6e6
AMPLITUDE, SIGMA, GAP = 60.0, 2.0, 4000
MAX_SAMPLES = 600000
BASE_L = (0, 1, 8, 9, 10, 25, 26, 41, 127, 128, 129, 200, 255)
EDGES = (64, 128, 192, 256)
NAME = {"T1": "T1", "C1A": "C1", "C1B": "C1", "S1": "S1"}


def air_length(mode, lfield):
    return lfield + 1 if mode == "C1B" else TR.frame_a_length(lfield)


def l_fields(mode):
    """The issue's list and, for every edge of the byte loop's trips, the longest telegram at or below it and the shortest above."""
    out = set(BASE_L)
    for edge in EDGES:
        below = [lf for lf in range(256) if air_length(mode, lf) <= edge]
        above = [lf for lf in range(256) if air_length(mode, lf) > edge]
        out.add(max(below))
        if above:
            out.add(min(above))
    return sorted(out)


def air_bytes(mode, lfield, seed=0):
    rng = np.random.default_rng([77, TR.MODES.index(mode), lfield, seed])
    if mode == "C1B":
        return TR.frame_b(lfield + 1, rng.integers(0, 256, 256, dtype=np.uint8).tobytes())
    tel = bytearray(rng.integers(0, 256, lfield + 1, dtype=np.uint8).tobytes())
    tel[0] = lfield
    return TR.frame_a(tel)


def samples_of(mode, n_air):
    chips = len(TR.preamble(mode)) + len(TR.body(mode, bytes(n_air))) + 8
    return GAP + int(chips * FS / TR.CHIP_RATE[mode])


def capture_plan():
    """{name: [(mode, L-field)]}: one capture per mode; S1 in as many as keep each below MAX_SAMPLES."""
    plan = {m: [(m, lf) for lf in l_fields(m)] for m in ("T1", "C1A", "C1B")}
    part, size, k = [], 0, 0
    for lf in l_fields("S1"):
        n = samples_of("S1", air_length("S1", lf))
        if part and size + n > MAX_SAMPLES:
            plan[f"S1.{k}"] = part; part, size, k = [], 0, k + 1
        part.append(("S1", lf)); size += n
    plan[f"S1.{k}"] = part
    return plan


PLAN = capture_plan()
CAPTURES = sorted(PLAN)
_CACHE = {}


def capture(name):
    if ("cu8", name) not in _CACHE:
        _CACHE[("cu8", name)] = TR.modulate([(m, air_bytes(m, lf)) for m, lf in PLAN[name]], seed=CAPTURES.index(name), fs=FS, amplitude=AMPLITUDE,
                                            sigma=SIGMA, gap=GAP)
    return _CACHE[("cu8", name)]


def oracle_text(oracle, key, cu8):
    if ("text", key) not in _CACHE:
        _CACHE[("text", key)] = oracle.run(cu8, oracle.make_opts())["text"]
    return _CACHE[("text", key)]


def expected_lines(telegrams):
    """(mode name, CRC flag, hex) of every telegram that a receiver prints, from the restatement alone."""
    out = []
    for mode, air in telegrams:
        fb = mode == "C1B"
        out.append((NAME[mode], str(int(TR.crc_clean(fb, air, len(air)))), "0x" + TR.printed_hex(fb, air, len(air))))
    return out


def fields(text, tag):
    return [(f[1], f[2], f[8]) for f in (ln.split(";") for ln in text.splitlines()) if f[0] == tag]


# ---- the damaged telegrams that can be made on air ------------------------------------------------------------------------------
def damaged_telegrams():
    """[(label, mode, what modulate() takes, keep)]"""
    def flip(air, byte):
        out = bytearray(air); out[byte] ^= 0x10
        return bytes(out)
    a = air_bytes("T1", 50, 1)                               # 59 air bytes: blocks of 12, 18, 18 and 11
    assert TR.blocks(False, len(a)) == [(0, 12), (12, 18), (30, 18), (48, 11)]
    b = air_bytes("C1B", 150, 1)                             # 151 air bytes: blocks of 128 and 23
    s = air_bytes("S1", 20, 1)
    sym = TR.body("T1", a); sym[12 * 20:12 * 20 + 6] = [1, 1, 1, 0, 0, 0]            # data byte 20, high symbol: 111000 is no 3-out-of-6 symbol
    pair = TR.body("S1", s); pair[16 * 7 + 4:16 * 7 + 6] = [0, 0]
    assert 0b111000 in TR.INVALID_SYMBOLS
    return [("clean T1", "T1", a, 1.0), ("A first", "T1", flip(a, 5), 1.0), ("A middle", "T1", flip(a, 20), 1.0), ("A last", "T1", flip(a, 50), 1.0),
            ("clean C1B", "C1B", b, 1.0), ("B first", "C1B", flip(b, 60), 1.0), ("B last", "C1B", flip(b, 140), 1.0),
            ("3of6", "T1", sym, 1.0), ("clean S1", "S1", s, 1.0), ("pair", "S1", pair, 1.0), ("half", "T1", air_bytes("T1", 60, 2), 0.5),
            ("clean C1A", "C1A", air_bytes("C1A", 30, 1), 1.0)]


def damaged_capture():
    if "damaged" not in _CACHE:
        _CACHE["damaged"] = TR.modulate([(m, w, k) for _, m, w, k in damaged_telegrams()], seed=99, fs=FS, amplitude=AMPLITUDE, sigma=SIGMA, gap=GAP)
    return _CACHE["damaged"]


# ---- the precondition, without a GPU ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CAPTURES)
def test_the_oracle_prints_every_telegram_of_every_capture(oracle, name):
    """Both framers' lines for EVERY telegram, in order: the mode, the restated CRC verdict (set exactly where the telegram has at least
    12 air bytes and every block has room for its CRC) and the restated CRC-free hex."""
    cu8 = capture(name)
    assert cu8.size % 4096 == 0 and cu8.size // 2 <= MAX_SAMPLES + 2 * GAP + 4096
    text = oracle_text(oracle, name, cu8)
    want = expected_lines([(m, air_bytes(m, lf)) for m, lf in PLAN[name]])
    assert len(want) >= 2
    assert fields(text, "rla") == want
    assert fields(text, "t2a") == want
    assert len(text.splitlines()) == 2 * len(want)
    assert all(ln.split(";")[3] == "1" for ln in text.splitlines())


def test_the_plan_covers_the_edges_of_the_byte_loop():
    for mode in TR.MODES:
        lengths = {air_length(mode, lf) for lf in l_fields(mode)}
        want = {64, 65, 128, 129, 192, 193, 256} if mode == "C1B" else {64, 65, 128, 129, 192, 195, 256, 257}
        assert want <= lengths, (mode, sorted(lengths))
        assert set(BASE_L) <= set(l_fields(mode))
    assert sorted(lf for name in CAPTURES if name.startswith("S1") for _, lf in PLAN[name]) == l_fields("S1")


def test_the_oracle_on_the_damaged_capture(oracle):
    """A flipped bit costs the CRC flag and nothing else; the invalid 3-out-of-6 symbol shows in its flag; the invalid Manchester pair
    and the carrier that stops half way print nothing."""
    text = oracle_text(oracle, "damaged", damaged_capture())
    want = []
    for label, mode, what, keep in damaged_telegrams():
        if label in ("pair", "half"):
            continue
        if label == "3of6":
            a = bytearray(air_bytes("T1", 50, 1)); a[20] = 0xFF
            want.append(("T1", "0", "0", "0x" + TR.printed_hex(False, a, len(a))))
        else:
            want.append(expected_lines([(mode, what)])[0][:2] + ("1", expected_lines([(mode, what)])[0][2]))
    for tag in ("rla", "t2a"):
        got = [(f[1], f[2], f[3], f[8]) for f in (ln.split(";") for ln in text.splitlines()) if f[0] == tag]
        assert got == want, tag
    assert [w[1] for w in want] == ["1", "0", "0", "0", "1", "0", "0", "0", "1", "1"]


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------
HOW = {"one push": dict(), "bursts to host": dict(bursts_to_host=True), "rssi on demand": dict(keep_taps=False), "pushes of 37 blocks": dict(push=37 * 4096)}


@pytest.mark.gpu
@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("name", CAPTURES)
def test_capture_decodes_to_the_oracles_text(wm, oracle, name, how):
    """One push with the debug taps (keep_taps, the default here): the kernel decodes every telegram.  bursts_to_host: the host
    decoders do.  keep_taps=False: RSSI on demand.  Pushes of 37 x 4096 bytes cut telegrams and continue them."""
    cu8 = capture(name)
    want = oracle_text(oracle, name, cu8)
    assert len(want.splitlines()) == 2 * len(PLAN[name])
    kw = dict(HOW[how]); push = kw.pop("push", cu8.size)
    with wm.Receiver(n_streams=1, max_push_bytes=push, **kw) as rx:
        assert rx.run(cu8, push_bytes=push)[0] == want


@pytest.mark.gpu
def test_t1_capture_in_pushes_of_one_block(wm, oracle):
    """4096 bytes are 2048 samples, 128 T1 chips: every telegram above 10 bytes is cut and continued, most of them many times."""
    cu8 = capture("T1")
    want = oracle_text(oracle, "T1", cu8)
    assert len(want.splitlines()) == 2 * len(PLAN["T1"])
    with wm.Receiver(n_streams=1, max_push_bytes=4096, keep_taps=False) as rx:
        assert rx.run(cu8, push_bytes=4096)[0] == want


S1_LONGEST = next(n for n in CAPTURES if ("S1", 255) in PLAN[n])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("name", ["T1", S1_LONGEST])
def test_segments_of_1024_samples_in_both_clock_forms(wm, oracle, name, waves):
    """seg_len = rla_seg_len = 1024 with short warm-ups: the 290-byte S1 telegram (226 000 samples at 1.6 MS/s) spans over a hundred
    segments of either framer, and k3_locate walks them."""
    cu8 = capture(name)
    want = oracle_text(oracle, name, cu8)
    assert len(want.splitlines()) == 2 * len(PLAN[name])
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, seg_len=1024, rla_seg_len=1024, warmup_t1c1=512, warmup_s1=512, clock_waves=waves) as rx:
        assert rx.run(cu8)[0] == want


@pytest.mark.gpu
def test_three_modes_side_by_side_in_one_context(wm, oracle):
    """Three captures of different modes, padded to one length with the idle level: every capture's text is its own."""
    names = ["T1", "C1B", S1_LONGEST]
    n = max(capture(x).size for x in names)
    caps = [np.concatenate([capture(x), np.full(n - capture(x).size, 128, np.uint8)]) for x in names]
    want = [oracle_text(oracle, ("padded", x, n), c) for x, c in zip(names, caps)]
    assert [len(w.splitlines()) for w in want] == [2 * len(PLAN[x]) for x in names]
    with wm.Receiver(n_streams=3, max_push_bytes=n, keep_taps=False) as rx:
        assert rx.run(caps) == want


@pytest.mark.gpu
def test_damaged_telegrams_and_only_crc_ok(wm, oracle):
    """The damaged capture prints the oracle's text; with only_crc_ok exactly the lines whose CRC flag is clear disappear."""
    cu8 = damaged_capture()
    want = oracle_text(oracle, "damaged", cu8)
    flags = [ln.split(";")[2] for ln in want.splitlines()]
    assert flags.count("1") == 8 and flags.count("0") == 12
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size) as rx:
        assert rx.run(cu8)[0] == want
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, only_crc_ok=True) as rx:
        assert rx.run(cu8)[0] == "".join(ln + "\n" for ln in want.splitlines() if ln.split(";")[2] == "1")
    with wm.Receiver(n_streams=1, max_push_bytes=37 * 4096, only_crc_ok=True, bursts_to_host=True) as rx:
        assert rx.run(cu8, push_bytes=37 * 4096)[0] == "".join(ln + "\n" for ln in want.splitlines() if ln.split(";")[2] == "1")
