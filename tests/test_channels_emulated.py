"""Several channels of one wideband capture in one context (cfg.input_channels): the ABI; the device source of the channels form of the
two K0-stage kernels (rtl-wmbus_amd/csrc/wm_k0_resample.h, k0_resample_block_t / k0_convert_block with CH = true, what k0_resample_ch<>
and k0_convert_ch<> run) on the coroutine block emulator, driven as wm_api.hip drives it -- the grid's y the pipeline stream, raw bytes
and level tables by capture -- against the single-shift restatements tests/shift_ref.py, dc_ref.py and agc_ref.py PER CHANNEL, byte for
byte and clip count for clip count; the 0 Hz identity; and the three-channel fixture of the GPU test through the oracle.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import channels_fixture as CF
import format_ref as FR
import shift_ref as SR
from test_dc_emulated import dc_inputs
from test_formats_emulated import FMT_IDS, FORMATS, RATES, design
from test_resample_emulated import BLK, CUTS, N_BLOCKS
from test_shift_emulated import shift_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libchannels_emu.so")
SRC = os.path.join(HERE, "emu", "channels_emu.cpp")

OUT_HZ = 1600000                                    # decimation 2
assert RATES == [0, 2048000, 2500000, 10000000]     # native (the conversion kernel), and three rates through the resampler
RATE_IDS = [str(r) if r else "native" for r in RATES]
LISTS = ["two", "edges", "twins"]                   # [+200000, -123457], [0, -Fin / 2, +1], [f, f]
GAINS = [256, 4096]


def fin_of(rate):
    return rate or OUT_HZ


def channel_list(name, rate):
    return {"two": [200000, -123457], "edges": [0, -(fin_of(rate) // 2), 1], "twins": [-123457, -123457]}[name]


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_channels: on a library without the fields no test of this file says anything, so none passes."""
    assert "input_channels" in [f[0] for f in wm.Cfg._fields_] and hasattr(wm.Line, "channel")


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    u, vp, sz = ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t
    L.wm_emu_ch_new.restype = vp
    L.wm_emu_ch_new.argtypes = [u] * 5 + [vp, u, u, u, vp, vp, u, u, u]
    L.wm_emu_ch_free.argtypes = [vp]
    L.wm_emu_ch_push.restype = ctypes.c_long
    L.wm_emu_ch_push.argtypes = [vp, vp, sz, sz, vp, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    L.wm_emu_ch_read_dc.restype = ctypes.c_long
    L.wm_emu_ch_read_dc.argtypes = [vp, u, vp, sz]
    L.wm_emu_ch_read_gain.restype = ctypes.c_long
    L.wm_emu_ch_read_gain.argtypes = [vp, u, vp, sz]
    L.wm_emu_ch_pick_tile.restype = u
    L.wm_emu_ch_pick_tile.argtypes = [u] * 3
    L.wm_emu_ch_convert_tile.restype = u
    L.wm_emu_ch_convert_tile.argtypes = [u]
    L.wm_emu_ch_max_channels.restype = u
    return L


def library_tile(emu, wm, fmt, rate):
    """The tile wmbus_open picks for the path: channels change neither."""
    if rate == 0:
        return emu.wm_emu_ch_convert_tile(fmt)
    L, M, T, _ = wm.resampler_design(rate, OUT_HZ)
    tile = emu.wm_emu_ch_pick_tile(L, M, T)
    assert tile > 0
    return tile


def run_emulated(emu, wm, caps, fmt, gain, fin, hz, L, M, taps, cuts, tile, R=0, agc=0):
    """caps: equally long raw captures.  Returns (bytes [capture][channel], the pushes' clip counts summed, dc [capture] int64 [n, 2] or
    None, gains [capture] int64 [n] or None): the level tables read push by push, by capture."""
    n_cap, n_ch = len(caps), len(hz)
    steps = np.array([wm.shift_design(fin, f)[0] for f in hz], np.uint32)
    table = wm.shift_design(fin, 0)[1]
    T = taps.shape[1] if taps is not None else 1
    tp = np.ascontiguousarray(taps, np.int16) if taps is not None else None
    max_blk = max(cuts) // FR.BPS[fmt] // 512
    h = emu.wm_emu_ch_new(fmt, gain, L, M, T, tp.ctypes.data if tp is not None else None, tile, n_cap, n_ch, steps.ctypes.data, table.ctypes.data,
                          R, agc, max_blk)
    assert h
    S = n_cap * n_ch
    got = [[] for _ in range(S)]
    dcs, gains = [[] for _ in range(n_cap)], [[] for _ in range(n_cap)]
    off = clipped = 0
    try:
        for n in cuts:
            raw = np.ascontiguousarray(np.stack([c[off:off + n] for c in caps])); off += n
            cap = BLK + 2 * FR.n_outputs(n // FR.BPS[fmt], L, M)
            win = np.full((S, cap + 64), 0xA5, np.uint8)
            clip = ctypes.c_uint32(0xFFFFFFFF)
            r = emu.wm_emu_ch_push(h, raw.ctypes.data, n, n, win.ctypes.data, cap + 64, cap, ctypes.byref(clip))
            assert r >= 0 and r % BLK == 0
            assert np.all(win[:, -64:] == 0xA5)              # nothing written past a stream's window
            for v in range(S):
                got[v].append(win[v, :r].copy())
            clipped += clip.value
            n_blk = n // FR.BPS[fmt] // 512
            for k in range(n_cap):
                if R:
                    t = np.full((n_blk + 1, 2), 0x7777, np.int16)
                    assert emu.wm_emu_ch_read_dc(h, k, t.ctypes.data, n_blk + 1) == n_blk and np.all(t[n_blk] == 0x7777)
                    dcs[k].append(t[:n_blk].astype(np.int64))
                if agc:
                    g = np.full(n_blk + 1, 0x7777, np.uint16)
                    assert emu.wm_emu_ch_read_gain(h, k, g.ctypes.data, n_blk + 1) == n_blk and g[n_blk] == 0x7777
                    gains[k].append(g[:n_blk].astype(np.int64))
    finally:
        emu.wm_emu_ch_free(h)
    assert off == caps[0].size
    out = [[np.concatenate(got[k * n_ch + c]) for c in range(n_ch)] for k in range(n_cap)]
    return (out, clipped, [np.concatenate(d) for d in dcs] if R else None, [np.concatenate(g) for g in gains] if agc else None)


def two_captures(raw, fmt):
    """The capture and its samples in reverse order: a v / C or stride mix-up between captures shows."""
    return [raw, np.ascontiguousarray(raw.reshape(-1, FR.BPS[fmt])[::-1].reshape(-1))]


def check(emu, wm, caps, fmt, gain, rate, hz, cut, tile, R=0, agc=0, tag=None):
    L, M, taps = design(wm, rate)
    fin = fin_of(rate)
    got, got_clips, got_dc, got_g = run_emulated(emu, wm, caps, fmt, gain, fin, hz, L, M, taps, CUTS[cut], tile, R, agc)
    clips = 0
    for k, raw in enumerate(caps):
        for c, f in enumerate(hz):
            want, n_clip, dc, g = CF.restated(raw, fmt, fin, f, gain, L, M, taps, R, agc)
            want = CF.whole_blocks(want)
            assert got[k][c].size == want.size, (tag, k, c)
            assert np.array_equal(got[k][c], want), (tag, k, c, int(np.argmax(got[k][c] != want)))
            clips += n_clip
            if R:                                            # one row per capture, what the single context computes
                assert np.array_equal(got_dc[k], dc), (tag, k)
            if agc:
                assert np.array_equal(got_g[k], g), (tag, k)
    assert got_clips == clips, tag                           # every channel's outputs counted, the ones behind the last whole block too
    return clips


# ---- 5. the ABI --------------------------------------------------------------------------------------------------------------------

def test_the_abi_has_the_channel_fields(wm, tmp_path):
    """Fails on a tree without the feature.  sizeof(wmbus_line) is what it was and `channel` sits where `pad` sat; the two configuration
    fields stand together, in front of the fields whose place from the end of the struct existing tests pin."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_channels")
    assert names[k + 1] == "input_channel_hz" and k + 1 < names.index("input_rate_hz")
    assert names[-5:] == ["input_rate_hz", "input_shift_hz", "input_dc", "input_format", "input_gain_q8"]       # the input stage's keep their order
    types = dict((f[0], f[1]) for f in wm.Cfg._fields_)
    assert types["input_channels"] is ctypes.c_uint and ctypes.sizeof(types["input_channel_hz"]) == 4 * 8 and wm.MAX_CHANNELS == 8
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(wmbus_line),offsetof(wmbus_line,channel),sizeof(((wmbus_line*)0)->channel),offsetof(wmbus_cfg,input_channels),'
                   'offsetof(wmbus_cfg,input_channel_hz),WMBUS_MAX_CHANNELS);return 0;}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [24, 7, 1]                             # 4 + 3 + 1 + 8 + 4 + 4: the size before the rename, pad's offset
    assert got[:2] == [ctypes.sizeof(wm.Line), wm.Line.pad.offset]          # the mirror stores the byte under its old name ...
    ln = wm.Line()
    ln.pad = 5
    assert ln.channel == 5                                   # ... and reads it as the channel
    assert got[3:5] == [wm.Cfg.input_channels.offset, wm.Cfg.input_channel_hz.offset] and got[5] == 8
    c = wm.Cfg()
    c.input_channels = 5
    c.input_channel_hz[7] = -1
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_channels == 0 and list(c.input_channel_hz) == [0] * 8
    c = wm._make_cfg(input_channel_hz=[325000, -325000])
    assert c.input_channels == 2 and list(c.input_channel_hz)[:3] == [325000, -325000, 0] and c.input_shift_hz == 0
    assert wm._make_cfg().input_channels == 0
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("#define WMBUS_MAX_CHANNELS 8", "unsigned input_channels;", "int input_channel_hz[WMBUS_MAX_CHANNELS];", "uint8_t  channel;",
                 "CHANNELS (cfg.input_channels = C", "pipeline stream v = k C + c"):
        assert word in hdr, word


def test_the_batch_plan_counts_captures(wm):
    """wmbus_batch_plan is unchanged: it splits captures, whatever the channels (no device needed)."""
    for n in (5, 64, 200, 1024):
        plain = wm._make_cfg(n_streams=n)
        chan = wm._make_cfg(n_streams=n, input_channel_hz=[325000, -325000, 0])
        out = [(ctypes.c_uint * n)(), (ctypes.c_uint * n)()]
        counts = [wm.lib().wmbus_batch_plan(ctypes.byref(c), 0, o, n) for c, o in zip((plain, chan), out)]
        assert counts[0] == counts[1] and list(out[0]) == list(out[1]) and sum(out[1]) == n


def test_refusals_that_need_no_device(wm):
    """wmbus_open looks at the configuration before it looks for a device: the three refusals name their field with or without a GPU.  A
    channel beyond Fin / 2 is also what wmbus_shift_design refuses."""
    with pytest.raises(wm.WmbusError, match="input_channels"):
        wm.Receiver(input_channel_hz=[1000 * k for k in range(9)])
    with pytest.raises(wm.WmbusError, match="input_shift_hz must be 0 with input_channels"):
        wm.Receiver(input_channel_hz=[325000, -325000], input_shift_hz=1000)
    with pytest.raises(wm.WmbusError, match=r"input_channel_hz\[1\] = -800001"):
        wm.Receiver(input_channel_hz=[800000, -800001])
    with pytest.raises(wm.WmbusError, match=r"input_channel_hz\[0\] = 1024001"):
        wm.Receiver(input_channel_hz=[1024001], input_rate_hz=2048000)
    with pytest.raises(wm.WmbusError):
        wm.shift_design(OUT_HZ, -800001)
    assert wm.shift_design(OUT_HZ, -800000)[0] == 1 << 31     # the edge itself is legal


# ---- 1. bytes and clip counts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cut", ["one", "uneven"])
@pytest.mark.parametrize("chans", LISTS)
@pytest.mark.parametrize("rate", RATES, ids=RATE_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement_per_channel(emu, wm, fmt, rate, chans, cut):
    hz = channel_list(chans, rate)
    caps = two_captures(shift_inputs(fmt, N_BLOCKS * BLK)["random"], fmt)
    tile = library_tile(emu, wm, fmt, rate)
    clip_seen = 0
    for g in GAINS:
        clip_seen += check(emu, wm, caps, fmt, g, rate, hz, cut, tile, tag=(g,))
    assert clip_seen > 0                                     # the output clamp is reached


@pytest.mark.parametrize("rate", [0, 2500000], ids=["native", "2500000"])
def test_result_does_not_depend_on_the_tile(emu, wm, rate):
    """Small tiles: many blocks per stream, so that a block's capture and channel are worked out at every block index."""
    caps = two_captures(shift_inputs(FR.CS16, N_BLOCKS * BLK)["random"], FR.CS16)
    for tile in (72, 1000) if rate == 0 else (64, 190):
        check(emu, wm, caps, FR.CS16, 4096, rate, [200000, 0, -123457], "uneven", tile, tag=tile)


def test_eight_channels_and_three_captures(emu, wm):
    """The most channels a context takes, every one with its own step, beside a capture count that is no power of two."""
    assert emu.wm_emu_ch_max_channels() == wm.MAX_CHANNELS == 8
    raw = shift_inputs(FR.CS8, N_BLOCKS * BLK)["random"]
    caps = two_captures(raw, FR.CS8) + [np.roll(raw, 2 * 1237)]
    hz = [0, 100000, -100000, 200000, -200000, 300000, -300000, 800000]
    check(emu, wm, caps, FR.CS8, 4096, 0, hz, "uneven", 1000)
    check(emu, wm, caps, FR.CS8, 256, 2048000, [h * 5 // 4 for h in hz], "one", library_tile(emu, wm, FR.CS8, 2048000))


# ---- 2. a 0 Hz channel is the unshifted rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", [0, 2048000, 4000000], ids=["native", "2048000", "4000000"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_a_0_hz_channel_is_the_unshifted_rule(emu, wm, fmt, rate):
    """The rotating rule with f = 0 -- step 0, table entry 0 = {16384, 0}, cu8 / cs8 widened x 64 with F = 21 -- gives the bytes and the clip
    count of format_ref.convert; with the blocker and with the AGC those of dc_ref.convert / agc_ref.convert with f = 0.  First on the
    restatements, then on the device source."""
    import agc_ref as AR
    import dc_ref as DR
    step, table = wm.shift_design(fin_of(rate), 0)
    assert step == 0 and table[0].tolist() == [16384, 0]
    L, M, taps = design(wm, rate)
    fin = fin_of(rate)
    raw = shift_inputs(fmt, N_BLOCKS * BLK)["random"]
    tile = library_tile(emu, wm, fmt, rate)
    for g in (77, 256, 4096):
        want, clips = FR.convert(raw, fmt, g, L, M, taps)
        got, got_clips = SR.convert(raw, fmt, fin, 0, g, L, M, taps)
        assert np.array_equal(got, want) and got_clips == clips, g
        out, emu_clips, _, _ = run_emulated(emu, wm, [raw], fmt, g, fin, [0], L, M, taps, CUTS["uneven"], tile)
        assert np.array_equal(out[0][0], CF.whole_blocks(want)) and emu_clips == clips, g
    off = dc_inputs(fmt, N_BLOCKS * BLK)["offset"]
    want, clips, dc = DR.convert(off, fmt, 6, 0, 0, 4096, L, M, taps)
    out, emu_clips, emu_dc, _ = run_emulated(emu, wm, [off], fmt, 4096, fin, [0], L, M, taps, CUTS["uneven"], tile, R=6)
    assert np.array_equal(out[0][0], CF.whole_blocks(want)) and emu_clips == clips and np.array_equal(emu_dc[0], dc)
    want, clips, g = AR.convert(off, fmt, 0, 0, 0, L, M, taps)
    out, emu_clips, _, emu_g = run_emulated(emu, wm, [off], fmt, 12345, fin, [0], L, M, taps, CUTS["uneven"], tile, agc=1)
    assert np.array_equal(out[0][0], CF.whole_blocks(want)) and emu_clips == clips and np.array_equal(emu_g[0], g)


# ---- 3. the blocker and the AGC: per capture, in front of the rotation -----------------------------------------------------------

@pytest.mark.parametrize("mode", ["dc", "agc", "both"])
@pytest.mark.parametrize("rate", [0, 2048000, 2500000], ids=["native", "2048000", "2500000"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_blocker_and_agc_are_per_capture(emu, wm, fmt, rate, mode):
    """Two captures with different offsets and levels, three channels (0 Hz among them): every channel's bytes are the single-shift
    restatement's, and the DC and gain tables have one row per capture, equal to the single context's."""
    named = dc_inputs(fmt, N_BLOCKS * BLK)
    caps = [named["offset"], named["step"]]
    R, agc = (6 if mode != "agc" else 0), (1 if mode != "dc" else 0)
    gain = 12345 if agc else 4096                            # an AG stage must not look at K0Args.gain_q8
    for cut in ("one", "uneven"):
        check(emu, wm, caps, fmt, gain, rate, [200000, 0, -123457], cut, library_tile(emu, wm, fmt, rate), R, agc, tag=(mode, cut))


# ---- 4. the fixture of the GPU test ------------------------------------------------------------------------------------------------

def test_three_channel_capture_decodes_on_every_channel(wm, oracle):
    """The 4.0 MS/s cs16 capture of tests/channels_fixture.py at gain 409: the oracle on shift_ref.pipeline_bytes per channel gives at
    least 6 lines on every channel -- the count of each capture alone, worked out on the CPU: 8, 10 and 6 -- with no byte clipped, and no
    line's text appears on another channel."""
    raw, parts = CF.wideband(wm)
    assert raw.size == 4 * CF.WIDE_N
    L, M, T, taps = wm.resampler_design(CF.WIDE_FS, OUT_HZ)
    assert (L, M, T) == (2, 5, 48)
    texts = []
    for f in CF.WIDE_HZ:
        y, clips = SR.convert(raw, FR.CS16, CF.WIDE_FS, f, CF.WIDE_GAIN, L, M, taps)
        assert clips == 0
        texts.append(oracle.run(np.ascontiguousarray(CF.whole_blocks(y)), oracle.make_opts())["text"].splitlines())
    counts = [len(t) for t in texts]
    print("lines per channel:", counts)
    assert all(n >= 6 for n in counts)
    assert counts == CF.WIDE_LINES
    for a in range(3):
        for b in range(a + 1, 3):
            assert not set(texts[a]) & set(texts[b])
