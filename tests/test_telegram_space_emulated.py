"""k3_bursts (device source rtl-wmbus_amd/csrc/wm_k3_bursts.h) over the whole telegram space, on the coroutine block emulator.

Chip streams are written by hand into the time2 regions: every L-field of every mode, telegrams with one damaged bit, symbol, pair,
RSSI byte or framer reset, streams cut into segments at chosen places, several captures, arenas that are too small.  Every WmPkt the
kernel writes is held, field by field, against tests/telegram_ref.py::expect (a restatement that shares no code with the product) AND
against the product's host decoder wm_decoder.c fed the same chips; the line formatted from the kernel's packet must be the line the
host decoder formats.  The reference's own packet decoders have answered the same streams once (ref_probe chips): the sha256 of
their text is in tests/golden/reference_outputs.json, and the kernel's and the host decoder's lines must hash to it.  No GPU needed."""
import ctypes
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_ffi as O
import telegram_ref as TR
import test_burst_need as BN
from test_k3_emulated import F_RLA, F_S1, F_T1C1, F_T2A, HDR, PKT, emu_k3  # noqa: F401  (emu_k3: a fixture)

emu_need = BN.emu
LIMIT = 16 * 290 + 2                     # chips a decoder can take from an access code on, and one more
ERR_BURST_OVERFLOW = 4                   # WM_ERR_BURST_OVERFLOW (wm_dev.h)
GUARD = 0xA5


@pytest.fixture(scope="module")
def emu(emu_k3, emu_need):
    k3, dec = emu_k3, emu_need
    k3.wm_emu_k3_captures.restype = ctypes.c_long
    k3.wm_emu_k3_captures.argtypes = [ctypes.c_uint, ctypes.c_void_p] + [ctypes.c_void_p] * 10 + [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    k3.wm_emu_k3_set_spans.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    dec.wm_emu_decode_burst.restype = ctypes.c_uint
    dec.wm_emu_decode_burst.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    dec.wm_decoder_format.restype = ctypes.c_size_t
    dec.wm_decoder_format.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    dec.wm_packet_format.restype = ctypes.c_size_t
    dec.wm_packet_format.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    dec.wm_packet_crc_ok.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int]
    return SimpleNamespace(k3=k3, dec=dec)


# ---- chip streams written by hand ---------------------------------------------------------------------------------------------
SEPARATOR = [4] + [0, 1] * 4             # between telegrams: a chip with the framer's reset marker, idle chips


class Streams:
    """The time2 chip regions and RSSI rows of S captures (`_hand_made_stream` of test_k3_emulated.py, grown to several captures
    and segments).  Chips of (capture, chain) are appended with put(); build() lays them into segments -- `spacing` samples apart,
    filling each segment unless `layout[(capture, chain)]` gives the chips per segment -- and draws the RSSI rows: seeded random
    bytes at or above the decoders' gate, different in every capture and at every sample, so that a read of the wrong row or sample
    shows.  set_rssi() then overwrites the row at one chip's sample."""

    def __init__(self, S=1, seg_len=32768, spacing=4, seed=1, layout=None):
        self.S, self.seg_len, self.spacing, self.seed, self.layout = S, seg_len, spacing, seed, layout or {}
        self.vals = {(s, ch): [] for s in range(S) for ch in (0, 1)}
        self.telegrams = []

    def put(self, s, ch, vals, label=None, mode=None):
        """Appends the chips; returns the index of the first one.  With a label the chips are a telegram that the checks look at."""
        flat = self.vals[(s, ch)]
        chip0 = len(flat)
        flat.extend(int(v) for v in vals)
        if label is not None:
            self.telegrams.append(SimpleNamespace(label=label, mode=mode, s=s, ch=ch, chip0=chip0))
        return chip0

    def build(self):
        S, seg_len = self.S, self.seg_len
        per_seg = seg_len // self.spacing - 1
        cap1 = seg_len // 4 + 8
        counts = {}
        for key, flat in self.vals.items():
            c = list(self.layout.get(key, []))
            left = len(flat) - sum(c)
            assert left >= 0 and all(x <= per_seg for x in c)
            while left > 0:
                c.append(min(per_seg, left)); left -= c[-1]
            counts[key] = c
        nseg1 = max(1, max(len(c) for c in counts.values()))
        seg0, nseg0, cap0 = 8192, 1, 8192 // 2 + 8
        M = nseg1 * seg_len; Mcap = (M + 255) // 256 * 256
        self.chips1 = np.zeros((2, S, nseg1, cap1), np.uint32); self.counts1 = np.zeros((2, S, nseg1), np.uint32); self.seen1 = np.zeros((2, S, nseg1), np.uint32)
        self.chips0 = np.zeros((2, S, nseg0, cap0), np.uint32); self.counts0 = np.zeros((2, S, nseg0), np.uint32); self.seen0 = np.zeros((2, S, nseg0), np.uint32)
        self.rssi = np.random.default_rng(self.seed).integers(TR.RSSI_GATE, 256, (2, S, Mcap)).astype(np.uint8)
        self.pm, self.v = {}, {}
        for (s, ch), flat in self.vals.items():
            v = np.asarray(flat, np.uint32).reshape(-1)
            pm = np.zeros(v.size, np.int64)
            at = 0
            for sg, c in enumerate(counts[(s, ch)]):
                pos = self.spacing * np.arange(c, dtype=np.uint32) + 1
                self.chips1[ch, s, sg, :c] = (pos << 3) | v[at:at + c]
                self.counts1[ch, s, sg] = c; self.seen1[ch, s, sg] = c > 0
                pm[at:at + c] = sg * seg_len + pos
                at += c
            self.pm[(s, ch)], self.v[(s, ch)] = pm, v
        self.geo = np.array([M, Mcap, F_T1C1 | F_S1 | F_RLA | F_T2A, 0, seg0, seg_len, nseg0, nseg1, cap0, cap1], np.uint64)
        self.M, self.Mcap = M, Mcap
        return self

    def set_rssi(self, s, ch, chip, value):
        self.rssi[ch, s, self.pm[(s, ch)][chip]] = value

    def chip_rssi(self, s, ch):
        return self.rssi[ch, s, self.pm[(s, ch)]]


def run_k3(emu, st, pkts_cap=None, bytes_cap=None, spans=True):
    """k3_scan, k3_spans (RSSI on demand, as the product runs) and k3_bursts with decode on.  The packet and byte arenas lie between
    guard bytes.  Returns hdr, words, the pkts array (whole, beyond the counter too), the byte arena, the kernels' error word, the
    packet counter and the two guarded buffers."""
    n_t = sum(int((v & 2).astype(bool).sum()) for v in st.v.values())
    pkts_cap = n_t + 8 if pkts_cap is None else pkts_cap
    bytes_cap = 296 * (n_t + 1) if bytes_cap is None else bytes_cap
    G = 256
    pk_buf = np.full(2 * G + pkts_cap * PKT.itemsize, GUARD, np.uint8)
    by_buf = np.full(2 * G + bytes_cap, GUARD, np.uint8)
    hdr = np.zeros(n_t + 8, HDR); words = np.zeros(LIMIT * 8 + 64, np.uint32); nw = ctypes.c_uint(0); npk = ctypes.c_uint(0); err = ctypes.c_uint(0)
    ntiles = (st.M + 975) // 976
    flags = np.zeros(ntiles * st.S, np.uint32)
    emu.k3.wm_emu_k3_set_spans(flags.ctypes.data if spans else None, ntiles if spans else 0)
    emu.k3.wm_emu_k3_set_spill(None, 0, None, None, None)
    emu.k3.wm_emu_k3_set_decode(pk_buf.ctypes.data + G, pkts_cap, ctypes.addressof(npk), by_buf.ctypes.data + G, bytes_cap)
    pend = np.zeros(4 * st.S, np.uint32)
    n = emu.k3.wm_emu_k3_captures(st.S, ctypes.addressof(err), st.geo.ctypes.data, st.chips0.ctypes.data, st.chips1.ctypes.data, st.counts0.ctypes.data,
                                  st.counts1.ctypes.data, st.seen0.ctypes.data, st.seen1.ctypes.data, st.rssi.ctypes.data, pend.ctypes.data,
                                  hdr.ctypes.data, hdr.size, words.ctypes.data, words.size, ctypes.byref(nw), 256)
    emu.k3.wm_emu_k3_set_decode(None, 0, None, None, 0)
    emu.k3.wm_emu_k3_set_spans(None, 0)
    assert n >= 0, n
    pkts = pk_buf[G:G + pkts_cap * PKT.itemsize].view(PKT)
    return SimpleNamespace(hdr=hdr[:n], words=words[:nw.value], pkts=pkts, n_pkts=npk.value, bytes=by_buf[G:G + bytes_cap], err=err.value,
                           guards=(pk_buf, by_buf, G))


def guards_intact(r):
    pk_buf, by_buf, G = r.guards
    return bool((pk_buf[:G] == GUARD).all() and (pk_buf[-G:] == GUARD).all() and (by_buf[:G] == GUARD).all() and (by_buf[-G:] == GUARD).all())


def host_decoder(emu, chain, vals, rssi, tag=b"t2a;"):
    """wm_decoder.c from the access-code chip vals[0] on.  None: the stream ended first."""
    dec = emu.dec
    buf = ctypes.create_string_buffer(dec.wm_emu_decoder_bytes())
    v8, r8 = np.ascontiguousarray(vals, np.uint8), np.ascontiguousarray(rssi, np.uint8)
    done = ctypes.c_int(0)
    k = dec.wm_emu_decode_burst(chain, v8.ctypes.data, r8.ctypes.data, v8.size, buf, ctypes.byref(done))
    if k == 0:
        return None
    out = dict(consumed=k, done=bool(done.value))
    if done.value:
        d = np.frombuffer(buf.raw, np.uint8)
        # wm_decoder (wm_decoder.h): step u16, mode u8, err3of6 u8, c1 u8, frame_b u8, l u16, L u16, [pad], sym u32, mode_bits u32, pkt_rssi u32, packet[292]
        l_ = int(d[6]) | int(d[7]) << 8
        out.update(err3of6=bool(d[3]), c1=bool(d[4]), frame_b=bool(d[5]), L=int(d[8]) | int(d[9]) << 8, bytes=bytes(d[24:24 + l_]),
                   pkt_rssi=int(np.frombuffer(buf.raw[20:24], "<u4")[0]), rssi_now=int(r8[k - 1]))
        out["crc_ok"] = bool(dec.wm_packet_crc_ok(ctypes.addressof(buf) + 24, out["L"], int(out["frame_b"])))
        line = ctypes.create_string_buffer(1024)
        ok = ctypes.c_int(-1)
        n = dec.wm_decoder_format(buf, tag, b"TS", out["rssi_now"], line, 1024, ctypes.byref(ok))
        out["line"] = line.raw[:n].decode()
        assert bool(ok.value) == out["crc_ok"]
    return out


def kernel_line(emu, p, arena, tag=b"t2a;"):
    """The line of a WmPkt as the product's host formats it (decode_stream_range, wm_host_decode.h): the stored bytes in a zeroed buffer."""
    nb = min(max(int(p["L"]), 2), 292)
    pkt = np.zeros(296, np.uint8)
    pkt[:nb] = arena[int(p["off"]):int(p["off"]) + nb]
    fl = int(p["flags"])
    line = ctypes.create_string_buffer(1024)
    n = emu.dec.wm_packet_format(int(p["chain"]), fl & 1, (fl >> 1) & 1, (fl >> 2) & 1, (fl >> 3) & 1, int(p["L"]), pkt.ctypes.data, int(p["pkt_rssi"]),
                                 int(p["rssi_now"]), tag, b"TS", line, 1024)
    return line.raw[:n].decode()


def check(emu, st, r):
    """Every telegram of the streams: the kernel's record against the restatement and against the host decoder.  Returns
    {label: result}; a result carries the packet's fields (`p`), the restatement's (`e`) and the line."""
    assert r.err == 0 and r.n_pkts <= len(r.pkts) and guards_intact(r)
    pkts = r.pkts[:r.n_pkts]
    by_key = {(int(p["stream"]), int(p["chain"]), int(p["chip0"])): p for p in pkts}
    hdr_key = {(int(h["stream"]), int(h["chain"]), int(h["chip0"])): h for h in r.hdr}
    assert len(by_key) == len(pkts) and len(hdr_key) == len(r.hdr)
    assert (pkts["algo"] == 1).all() and len(by_key) + len(hdr_key) == len(st.telegrams)          # every access code exactly once
    out = {}
    for t in st.telegrams:
        v, rs, pm = st.v[(t.s, t.ch)], st.chip_rssi(t.s, t.ch), st.pm[(t.s, t.ch)]
        sl = slice(t.chip0, t.chip0 + LIMIT)
        resets = np.nonzero(v[sl] & 4)[0].tolist()
        e = TR.expect(t.mode, v[sl], rs[sl], resets)
        h = host_decoder(emu, t.ch, v[sl], rs[sl])
        key = (t.s, t.ch, t.chip0)
        where = (t.label, t.mode)
        if e is None:                                        # the plan reaches past the stream: shipped as chips, all there are
            assert key in hdr_key and key not in by_key, where
            hd = hdr_key[key]
            avail = v.size - t.chip0
            assert (int(hd["n_chips"]), int(hd["avail"]), int(hd["flags"]), int(hd["pos0"])) == (avail, avail, 0, int(pm[t.chip0])), where
            want = ((pm[t.chip0:] - pm[t.chip0]).astype(np.uint32) << 11) | (rs[t.chip0:].astype(np.uint32) << 3) | (v[t.chip0:] & 7)
            assert np.array_equal(r.words[int(hd["word_off"]):int(hd["word_off"]) + avail], want), where
            out[t.label] = SimpleNamespace(p=None, e=None, h=h, hdr=hd, line=None, t=t)
            continue
        assert key in by_key and h is not None, where
        p = by_key[key]
        fl = int(p["flags"])
        assert int(p["consumed"]) == e["consumed"] == h["consumed"], (where, p, e, h)
        assert (int(p["status"]) == 1) == e["done"] == h["done"] and int(p["status"]) in (1, 2), (where, p, e, h)
        line = None
        if e["done"]:
            got = dict(L=int(p["L"]), c1=bool(fl & 1), frame_b=bool(fl & 2), err3of6=bool(fl & 4), crc_ok=bool(fl & 8),
                       bytes=bytes(r.bytes[int(p["off"]):int(p["off"]) + len(e["bytes"])]), pkt_rssi=int(p["pkt_rssi"]), rssi_now=int(p["rssi_now"]))
            for f, g in got.items():
                assert g == e[f], (where, f, g, e[f])
                assert g == h[f], (where, f, g, h[f])
            assert int(p["sample"]) == int(pm[t.chip0 + e["consumed"] - 1]), where
            line = kernel_line(emu, p, r.bytes)
            assert line == h["line"], where
            f = line.rstrip("\n").split(";")
            hexd = TR.printed_hex(e["frame_b"], e["bytes"], e["L"])
            assert f[:7] == ["t2a", "S1" if t.ch else "C1" if e["c1"] else "T1", str(int(e["crc_ok"])), "1" if t.ch else str(int(not e["err3of6"])),
                             "TS", str(e["pkt_rssi"]), str(e["rssi_now"])] and f[8] == "0x" + hexd, (where, line)
        else:
            assert not fl & 8, where                         # an abort carries no CRC verdict
        out[t.label] = SimpleNamespace(p=p, e=e, h=h, hdr=None, line=line, t=t)
    return out


def lines_of(res):
    """The lines of the results, in stream order."""
    done = sorted((x for x in res.values() if x.line is not None), key=lambda x: x.t.chip0)
    return [x.line.rstrip("\n") for x in done]


# ---- telegrams ------------------------------------------------------------------------------------------------------------------
def payload(mode, lfield, seed=0):
    """Seeded air bytes of a well-formed telegram of `mode` with that L-field."""
    rng = np.random.default_rng([TR.MODES.index(mode), lfield, seed])
    if mode == "C1B":
        return TR.frame_b(lfield + 1, rng.integers(0, 256, 256, dtype=np.uint8).tobytes())
    tel = bytearray(rng.integers(0, 256, lfield + 1, dtype=np.uint8).tobytes())
    tel[0] = lfield
    return TR.frame_a(tel)


def flip(air, byte, bit):
    out = bytearray(air); out[byte] ^= 1 << bit
    return bytes(out)


def t1_with_symbol(air, byte, high, sym):
    """The chips of the T1 telegram with one six-chip symbol replaced."""
    c = TR.chips("T1", air)
    at = 1 + 12 * byte + (0 if high else 6)
    c[at:at + 6] = [(sym >> (5 - i)) & 1 for i in range(6)]
    return c


DAMAGE_A = 255                                               # frame A, L-field 255: 290 air bytes in 17 blocks
T1_LONG = 112                                                # T1, L-field 112: 129 air bytes
C1A_BITS = 26                                                # C1 frame A, L-field 26: 33 air bytes, blocks of 12, 18 and 3


def crc_damage_cases(mode):
    """(label, air) of the CRC-damage sweep: for every block one flipped data bit, then one flipped bit in each CRC byte."""
    airs = {"A": payload(mode, DAMAGE_A, 7)} if mode != "C1B" else {"B256": payload(mode, 255, 7), "B201": payload(mode, 200, 7)}
    out = []
    for name, air in airs.items():
        out.append((("crc", name, "clean"), air))
        for k, (start, blk) in enumerate(TR.blocks(mode == "C1B", len(air))):
            data = start + max(1, (blk - 2) // 2) if start == 0 else start + (blk - 2) // 2     # never the L-field
            for what, byte in (("data", data), ("crc_hi", start + blk - 2), ("crc_lo", start + blk - 1)):
                out.append((("crc", name, k, what), flip(air, byte, (k + byte) % 8)))
    return out


def space_stream(mode):
    """One concatenated stream per mode: the clean sweep over L-fields 0..255 and the mode's damaged telegrams, a reset marker and
    idle chips between telegrams.  Frame B with L-field 128 is NOT in it: its restated block list ends in a block of one byte, on which
    the reference's CRC check computes `length - 2` on a size_t of 1 and reads far out of bounds; that telegram is held against the
    restatement and the host decoder in test_frame_b_with_a_one_byte_tail_block."""
    ch = TR.CHAIN[mode]
    st = Streams(S=1, seed=10 + TR.MODES.index(mode))

    def put(label, chips_):
        st.put(0, ch, chips_, label, mode)
        st.put(0, ch, SEPARATOR)

    st.put(0, ch, SEPARATOR)
    for lf in range(256):
        if not (mode == "C1B" and lf == 128):
            put(("clean", lf), TR.chips(mode, payload(mode, lf)))
    for label, air in crc_damage_cases(mode):
        put(label, TR.chips(mode, air))
    if mode == "C1A":
        air = payload(mode, C1A_BITS, 3)
        assert len(air) == 33 and TR.blocks(False, 33) == [(0, 12), (12, 18), (30, 3)]
        put(("bits", "clean"), TR.chips(mode, air))
        for byte in range(1, 33):
            for bit in range(8):
                put(("bits", byte, bit), TR.chips(mode, flip(air, byte, bit)))
        for fb, word in ((0, 0x54C), (1, 0x543)):
            for nib in range(16):
                if nib != 0xD:
                    put(("trailer", fb, nib), [2] + TR._bits(word, 12) + TR._bits(nib, 4) + TR.body("T1", payload("T1", 20)))
    if mode == "T1":
        air = payload(mode, T1_LONG, 5)
        assert len(air) == 129
        put(("3of6", "clean"), TR.chips(mode, air))
        for byte in (1, 63, 64, 128):
            for high in (1, 0):
                for sym in range(64):
                    put(("3of6", byte, high, sym), t1_with_symbol(air, byte, high, sym))
        short = payload(mode, 12)
        for high in (1, 0):
            for sym in TR.INVALID_SYMBOLS:
                put(("lsym", high, sym), t1_with_symbol(short, 0, high, sym))
    if mode == "S1":
        air = payload(mode, 10, 2)
        assert len(air) == 15
        clean = TR.chips(mode, air)
        for k in range(8 * 15):
            for pair in ((0, 0), (1, 1)):
                c = list(clean); c[1 + 2 * k:3 + 2 * k] = pair
                put(("pair", k, pair[0]), c)
    return st.build()


_SPACE = {}


@pytest.fixture
def space(emu, request):
    """(streams, kernel result, checked results) of a mode's concatenated stream; made once per mode."""
    def get(mode):
        if mode not in _SPACE:
            st = space_stream(mode)
            r = run_k3(emu, st)
            _SPACE[mode] = (st, r, check(emu, st, r))
        return _SPACE[mode]
    return get


@pytest.mark.parametrize("mode", TR.MODES)
def test_clean_sweep_every_l_field_of_every_mode(space, mode):
    """4 modes x L-field 0..255: the kernel's record equals the restatement's and the host decoder's (check()); the CRC verdict is
    clear below 12 air bytes and set everywhere else; frame B L-fields 0 and 1 store two bytes; frame B L-field 129 ends in a block
    that is the CRC of nothing and reads clean."""
    st, r, res = space(mode)
    n = 0
    for lf in range(256):
        if mode == "C1B" and lf == 128:
            continue
        x = res[("clean", lf)]
        air_len = lf + 1 if mode == "C1B" else TR.frame_a_length(lf)
        assert x.e["done"] and x.e["L"] == air_len and not x.e["err3of6"], (mode, lf)
        assert bool(int(x.p["flags"]) & 8) == x.e["crc_ok"] == (air_len >= 12), (mode, lf)
        want = payload(mode, lf)
        if mode == "C1B" and lf < 2:
            assert len(x.e["bytes"]) == 2 and x.e["bytes"][:air_len] == want and int(x.p["consumed"]) == 1 + 16 + 16, lf
        else:
            assert x.e["bytes"] == want, (mode, lf)
        n += 1
    assert n == (255 if mode == "C1B" else 256)
    if mode == "C1B":
        tail = res[("clean", 129)].e["bytes"][128:]
        assert tail == b"\xff\xff" and int(res[("clean", 129)].p["flags"]) & 8


def test_frame_b_with_a_one_byte_tail_block(emu):
    """Frame B, L-field 128: 129 air bytes, the tail block has no room for a CRC.  The verdict is clear (restatement, host decoder and
    kernel agree: check()).  The reference is not asked: see space_stream.  The oracle has no chip-level entry; it meets this telegram on
    air, in the C1B capture of test_gpu_telegrams.py, where the CPU test holds its line (CRC flag clear) against the restatement."""
    st = Streams(seed=3)
    air = payload("C1B", 128)
    assert TR.blocks(True, 129) == [(0, 128), (128, 1)] and TR.crc_clean(True, air, 128)      # the first block alone is clean
    st.put(0, 0, TR.chips("C1B", air), "b128", "C1B")
    res = check(emu, st.build(), run_k3(emu, st))
    x = res["b128"]
    assert x.e["done"] and x.e["bytes"] == air and not x.e["crc_ok"] and not int(x.p["flags"]) & 8 and ";0;1;" in x.line


@pytest.mark.parametrize("mode", TR.MODES)
def test_crc_damage_changes_the_verdict_and_nothing_else(space, mode):
    """One flipped bit in the data, the high CRC byte and the low CRC byte of EVERY block: only WM_PKTF_CRC_OK changes."""
    st, r, res = space(mode)
    cases = crc_damage_cases(mode)
    assert len(cases) == (2 + 3 * 4 if mode == "C1B" else 1 + 3 * 17)
    clean = {}
    for label, air in cases:
        x = res[label]
        if label[2] == "clean":
            clean[label[1]] = x
            assert int(x.p["flags"]) & 8, label
            continue
        c = clean[label[1]]
        assert int(x.p["status"]) == 1 and int(x.p["consumed"]) == int(c.p["consumed"]) and int(x.p["L"]) == int(c.p["L"]), label
        assert int(x.p["flags"]) == int(c.p["flags"]) & ~8, label
        diff = [i for i, (a, b) in enumerate(zip(x.e["bytes"], c.e["bytes"])) if a != b]
        assert len(diff) == 1 and x.e["bytes"] == air, label


def test_every_single_bit_of_a_three_block_c1_telegram(space):
    """C1 frame A, L-field 26 (33 bytes: blocks of 12, 18 and a short one of 3): every bit of bytes 1..32 flipped, one at a time."""
    st, r, res = space("C1A")
    assert int(res[("bits", "clean")].p["flags"]) & 8
    for byte in range(1, 33):
        for bit in range(8):
            x = res[("bits", byte, bit)]
            assert int(x.p["status"]) == 1 and int(x.p["consumed"]) == 1 + 16 + 8 * 33 and not int(x.p["flags"]) & 8, (byte, bit)


def test_three_out_of_six_symbols_at_the_trips_of_the_byte_loop(space):
    """Each of the 64 six-chip symbols at the high and at the low position of data bytes 1, 63, 64 and the last one of a 129-byte T1
    telegram: the error flag, the stored byte (0xFF once a symbol is invalid) and the CRC verdict on the bytes as stored."""
    st, r, res = space("T1")
    air = payload("T1", T1_LONG, 5)
    n_bad = n_ok = 0
    for byte in (1, 63, 64, 128):
        for high in (1, 0):
            for sym in range(64):
                x = res[("3of6", byte, high, sym)]
                nib = TR.NIBBLE_OF_SYMBOL.get(sym)
                stored = 0xFF if nib is None else (nib << 4 | air[byte] & 15) if high else (air[byte] & 0xF0 | nib)
                want = bytearray(air); want[byte] = stored
                got = bytes(r.bytes[int(x.p["off"]):int(x.p["off"]) + 129])
                assert int(x.p["status"]) == 1 and got == bytes(want), (byte, high, sym)
                assert bool(int(x.p["flags"]) & 4) == (nib is None), (byte, high, sym)
                assert bool(int(x.p["flags"]) & 8) == TR.crc_clean(False, want, 129) == (stored == air[byte]), (byte, high, sym)
                n_bad += nib is None; n_ok += stored == air[byte]
    assert n_bad == 8 * 48 and n_ok == 8


def test_headers_that_are_no_headers_abort_where_the_decoder_sees_it(space):
    """An invalid L-field symbol that spells no C1 mode word: abort 12 chips behind the access code.  A C1 mode word with one of the
    15 wrong trailer nibbles: abort after 16."""
    res = space("T1")[2]
    for high in (1, 0):
        for sym in TR.INVALID_SYMBOLS:
            p = res[("lsym", high, sym)].p
            assert (int(p["status"]), int(p["consumed"])) == (2, 13), (high, sym)
    res = space("C1A")[2]
    n = 0
    for fb in (0, 1):
        for nib in range(16):
            if nib != 0xD:
                p = res[("trailer", fb, nib)].p
                assert (int(p["status"]), int(p["consumed"])) == (2, 17), (fb, nib)
                n += 1
    assert n == 30


def test_invalid_manchester_pair_at_every_position(space):
    """S1, L-field 10: 00 and 11 at every pair position, the L-field's pairs and the last pair included.  The decoder stops on the
    chip that completes the pair, the record is an abort and no line comes out."""
    st, r, res = space("S1")
    for k in range(8 * 15):
        for first in (0, 1):
            x = res[("pair", k, first)]
            assert (int(x.p["status"]), int(x.p["consumed"])) == (2, 2 * k + 3) and x.line is None, (k, first)


# ---- the reference's answer, recorded -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TR.MODES)
def test_the_references_decoders_print_the_same_lines(space, mode):
    """The mode's concatenated stream through `ref_probe chips` (the reference's own packet decoders), recorded in
    golden/reference_outputs.json as sha256 of its text: the lines formatted from the emulated kernel's packets and the host
    decoder's lines hash to the same value."""
    st, r, res = space(mode)
    ch = TR.CHAIN[mode]
    raw = np.stack([st.v[(0, ch)].astype(np.uint8), st.chip_rssi(0, ch)], axis=1).astype(np.uint8).tobytes()

    def live():
        out = subprocess.run([O.REF_PROBE, "chips", str(ch), "t2a;"], input=raw, capture_output=True, check=True).stdout
        lines = O.mask_ts(out).decode().splitlines()
        return {"input": O.sha256(raw), "n": len(lines), "output": O.sha256("\n".join(lines).encode())}
    want = O.reference_answer(f"ref_probe chips telegram-space {mode} t2a;", live)
    assert want["input"] == O.sha256(raw), "the stream is not the one the reference decoded"
    kernel = lines_of(res)
    host = [x.h["line"].rstrip("\n") for x in sorted((x for x in res.values() if x.h and x.h["done"]), key=lambda x: x.t.chip0)]
    assert len(kernel) == want["n"] > 256
    assert O.sha256("\n".join(kernel).encode()) == want["output"]
    assert O.sha256("\n".join(host).encode()) == want["output"]


# ---- RSSI gate, framer reset ----------------------------------------------------------------------------------------------------
def test_rssi_gate_at_the_trips_of_the_chip_loop(emu):
    """A T1 telegram of 181 chips; the RSSI row reads 4 (below the gate) or 5 at chip 0, 1, 63, 64, n - 2, n - 1.  Below the gate the
    decoder is not armed (chip 0: one chip consumed) or drops the telegram on that chip -- except on the completing chip n - 1, where the
    telegram still completes.  pkt_rssi is the row at chip 1, rssi_now the one at the last chip.
    (In the kernel the exemption `j + 1 < n || !plan.done` changes no output: at j = n - 1 the gate would set ev = min(ev, n), and ev never
    exceeds n.  Replacing it by `j < n` is therefore no mutant that a test can kill; the case at n - 1 pins the behaviour, not the clause.)"""
    air = payload("T1", 10)
    n = 1 + 12 * len(air)
    assert n > 128
    st = Streams(seed=4)
    where = (0, 1, 63, 64, n - 2, n - 1)
    for j in where:
        for level in (4, 5):
            st.put(0, 0, TR.chips("T1", air), (j, level), "T1")
    st.build()
    for t in st.telegrams:
        st.set_rssi(0, 0, t.chip0 + t.label[0], t.label[1])
    r = run_k3(emu, st)
    res = check(emu, st, r)
    for j in where:
        lo, hi = res[(j, 4)].p, res[(j, 5)].p
        assert int(hi["status"]) == 1 and int(hi["consumed"]) == n, j
        if j == n - 1:
            assert int(lo["status"]) == 1 and int(lo["consumed"]) == n and int(lo["rssi_now"]) == 4 and int(hi["rssi_now"]) == 5
        else:
            assert (int(lo["status"]), int(lo["consumed"])) == (2, j + 1), j
        if j == 1:
            assert int(hi["pkt_rssi"]) == 5
        t = res[(j, 5)].t
        rows = st.chip_rssi(0, 0)
        assert (int(hi["pkt_rssi"]), int(hi["rssi_now"])) == (int(rows[t.chip0 + 1]), int(rows[t.chip0 + n - 1])), j


def test_framer_reset_before_chip_j(emu):
    """The reset marker on chip 1, 63, 64 and n - 1 of a telegram: the decoder is reset before that chip, j chips consumed."""
    air = payload("T1", 10)
    n = 1 + 12 * len(air)
    st = Streams(seed=5)
    for j in (1, 63, 64, n - 1):
        c = TR.chips("T1", air); c[j] |= 4
        st.put(0, 0, c, j, "T1")
    res = check(emu, st.build(), run_k3(emu, st))
    for j in (1, 63, 64, n - 1):
        assert (int(res[j].p["status"]), int(res[j].p["consumed"])) == (2, j), j


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_a_telegram_across_segments_one_of_them_empty(emu):
    """Six segments of 1024 samples; the telegram starts in segment 2, runs through the EMPTY segment 3 and ends in segment 5."""
    air = payload("C1A", 50)
    c = TR.chips("C1A", air)
    st = Streams(seg_len=1024, seed=6, layout={(0, 0): [17, 0, 40, 0, 250]})
    st.put(0, 0, [0, 1] * 20)                                # 40 idle chips: the access code is chip 23 of segment 2
    st.put(0, 0, c, "t", "C1A")
    st.build()
    assert st.geo[7] == 6 and st.counts1[0, 0].tolist()[:5] == [17, 0, 40, 0, 250]
    first, last = st.pm[(0, 0)][40] // 1024, st.pm[(0, 0)][40 + 16 + 8 * len(air)] // 1024
    assert (first, last) == (2, 5)
    res = check(emu, st, run_k3(emu, st))
    assert int(res["t"].p["status"]) == 1 and int(res["t"].p["flags"]) & 8


def test_two_captures_with_their_own_rows_and_telegrams(emu):
    """Two captures in lock step, both chains: different telegrams and different RSSI rows; every packet carries its capture's bytes
    and its capture's RSSI pair (check() reads them from that capture's row)."""
    st = Streams(S=2, seg_len=4096, seed=7)
    st.put(0, 0, [0, 1] * 5)
    st.put(0, 0, TR.chips("T1", payload("T1", 30, 1)), "t1@0", "T1")
    st.put(1, 0, TR.chips("C1B", payload("C1B", 140, 1)), "c1b@1", "C1B")
    st.put(1, 0, TR.chips("C1A", payload("C1A", 9, 1)), "c1a@1", "C1A")
    st.put(0, 1, TR.chips("S1", payload("S1", 12, 1)), "s1@0", "S1")
    st.put(1, 1, [1, 0] * 7)
    st.put(1, 1, TR.chips("S1", payload("S1", 25, 1)), "s1@1", "S1")
    st.build()
    assert not np.array_equal(st.rssi[:, 0], st.rssi[:, 1])
    res = check(emu, st, run_k3(emu, st))
    assert all(int(x.p["status"]) == 1 and int(x.p["flags"]) & 8 for x in res.values()) and len(res) == 5
    assert len({(int(x.p["pkt_rssi"]), int(x.p["rssi_now"])) for x in res.values()}) == 5


def test_three_telegrams_back_to_back(emu):
    """No chip between a telegram's last chip and the next access code."""
    st = Streams(seed=8)
    for k, lf in enumerate((15, 0, 33)):
        st.put(0, 0, [2] + TR.body("T1", payload("T1", lf, 2)), k, "T1")
    st.put(0, 0, TR.IDLE_TAIL)
    res = check(emu, st.build(), run_k3(emu, st))
    assert [int(res[k].p["status"]) for k in range(3)] == [1, 1, 1]
    assert int(res[0].p["chip0"]) + int(res[0].p["consumed"]) == int(res[1].p["chip0"])


@pytest.mark.parametrize("mode", ["T1", "C1B", "S1"])
def test_a_stream_that_ends_with_the_telegram_or_one_chip_earlier(emu, mode):
    """The stream ends on the telegram's last chip (`need` chips behind the access code, need + 1 with it): the burst is decoded.
    One chip earlier it is shipped as chips, all there are, bit for bit (check())."""
    ch = TR.CHAIN[mode]
    c = [2] + TR.body(mode, payload(mode, 20, 4))
    for short in (0, 1):
        st = Streams(seed=9)
        st.put(0, ch, TR.IDLE_TAIL)
        st.put(0, ch, c[:len(c) - short], "t", mode)
        r = run_k3(emu, st.build())
        x = check(emu, st, r)["t"]
        if short:
            assert x.p is None and int(x.hdr["n_chips"]) == int(x.hdr["avail"]) == len(c) - 1 and r.n_pkts == 0
        else:
            assert int(x.p["status"]) == 1 and int(x.p["consumed"]) == len(c) and len(r.hdr) == 0


# ---- arenas ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pkts", "bytes"])
def test_arenas_with_room_for_k_of_m_telegrams(emu, which):
    """Eight telegrams, room for three records or for the bytes of three: WM_ERR_BURST_OVERFLOW is raised, every slot below
    min(counter, capacity) holds a whole record of one of the telegrams with its bytes in the arena, and nothing is written outside
    the arenas (guard bytes on both sides, and the slots above the counter keep their fill)."""
    st = Streams(seed=11)
    airs = [payload("T1", 20 + k, 6) for k in range(8)]
    for k, air in enumerate(airs):
        st.put(0, 0, TR.chips("T1", air), k, "T1")
    st.build()
    size = len(airs[0])
    r = run_k3(emu, st, pkts_cap=3 if which == "pkts" else 16, bytes_cap=4096 if which == "pkts" else 3 * ((size + 8 + 3) & ~3))
    assert r.err & ERR_BURST_OVERFLOW and guards_intact(r)
    n = min(r.n_pkts, len(r.pkts))
    assert 1 <= n <= 3 if which == "pkts" else 1 <= n < 8
    starts = {t.chip0: t.label for t in st.telegrams}
    seen = set()
    for p in r.pkts[:n]:
        k = starts[int(p["chip0"])]
        air = airs[k]
        assert k not in seen and int(p["status"]) == 1 and int(p["flags"]) == 8 and int(p["L"]) == len(air) and int(p["consumed"]) == 1 + 12 * len(air)
        assert int(p["off"]) + len(air) <= len(r.bytes) and bytes(r.bytes[int(p["off"]):int(p["off"]) + len(air)]) == air, k
        seen.add(k)
    assert (r.pkts[n:].view(np.uint8) == GUARD).all()
    used = np.zeros(len(r.bytes), bool)
    for p in r.pkts[:n]:
        used[int(p["off"]):int(p["off"]) + int(p["L"])] = True
    assert (r.bytes[~used] == GUARD).all()
