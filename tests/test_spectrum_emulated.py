"""The channel survey (cfg.input_spectrum): the ABI; the restatement tests/spectrum_ref.py against numpy's FFT; the device source of its kernel
(rtl-wmbus_amd/csrc/wm_k0_spectrum.h: k0_spectrum_block) on the coroutine block emulator against the restatement, array for array;
wmbus_spectrum_channels against the restated rule; and what the survey is for, through the oracle: a capture tuned off its channel decodes
nothing, the survey finds the transmitter, and decoding at the survey's offset brings the telegrams back.  No GPU needed."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import channels_fixture as CF
import format_ref as FR
import shift_ref as SR
import spectrum_ref as PR
from test_formats_emulated import FMT_IDS, FORMATS
from test_resample_emulated import BLK, CUTS, N_BLOCKS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libspectrum_emu.so")
SRC = os.path.join(HERE, "emu", "spectrum_emu.cpp")
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
FS = 1600000
MIXES = [200000, -43000, 60000, -30000]             # Hz the bundled capture is mixed by
NOISE_SIGMAS = [1, 3, 10, 30]


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.input_spectrum: on a library without the field no test of this file says anything, so none passes."""
    assert "input_spectrum" in [f[0] for f in wm.Cfg._fields_] and "wmbus_read_spectrum" in wm.EXPORTS and "wmbus_spectrum_channels" in wm.EXPORTS


def test_the_abi_has_the_spectrum_field(wm, tmp_path):
    """Fails on a tree without the feature.  The field sits directly in front of input_channels; wmbus_timing keeps its 152 bytes."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("input_spectrum")
    assert names[k - 1] == "k1_small_tile" and names[k + 1:k + 3] == ["input_channels", "input_channel_hz"]
    assert names[k + 3:] == ["k1_tiles_per_block", "input_agc", "clock_waves", "line_levels", "input_rate_hz", "input_shift_hz", "input_dc", "input_format", "input_gain_q8"]
    assert dict((f[0], f[1]) for f in wm.Cfg._fields_)["input_spectrum"] is ctypes.c_uint
    c = wm.Cfg()
    c.input_spectrum = 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_spectrum == 0
    assert wm._make_cfg(input_spectrum=1).input_spectrum == 1 and wm._make_cfg().input_spectrum == 0
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned input_spectrum;",
                 "long wmbus_read_spectrum(wmbus_ctx *ctx, unsigned stream, uint64_t *sum, uint32_t *peak, uint64_t *blocks, int reset);",
                 "typedef struct wmbus_channel_hit { int32_t offset_hz; uint32_t ratio_q8; uint32_t floor_peak, floor_mean; } wmbus_channel_hit;",
                 "int wmbus_spectrum_channels(unsigned in_hz, const uint64_t *sum, const uint32_t *peak, uint64_t blocks,",
                 "unsigned width_hz, unsigned min_ratio_q8, unsigned rel, wmbus_channel_hit *out, unsigned cap);",
                 "SPECTRUM (cfg.input_spectrum = 1",
                 "w[n]  = (16384 - c[2 n] + 1) >> 1",
                 "y[n]  = (v[n] w[n] + 8192) >> 14",
                 "t_re = (b_re c[i] + b_im s[i] + 8192) >> 14,   t_im = (b_im c[i] - b_re s[i] + 8192) >> 14",
                 "pw[j] = (z_re[j]^2 + z_im[j]^2) >> 16",
                 "bin   b = (j + 256) mod 512",
                 "sum[b] += pw (uint64),   peak[b] = max(peak[b], pw) (uint32),   blocks += 1",
                 "offset_hz = floor((2 num in_hz + 512 den) / (1024 den))",
                 "2^33 full-scale level blocks"):
        assert word in hdr, word
    assert hdr.index("unsigned k1_small_tile;") < hdr.index("unsigned input_spectrum;") < hdr.index("unsigned input_channels;")
    for name in ("wmbus_read_spectrum", "wmbus_spectrum_channels"):
        assert name in wm.EXPORTS and hasattr(wm.lib(), name)
    assert hasattr(wm.Receiver, "read_spectrum") and hasattr(wm, "spectrum_channels")
    # the C structs themselves: the field's place, and the size existing tests pin
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, input_spectrum), offsetof(wmbus_cfg, input_channels), sizeof(wmbus_channel_hit), sizeof(wmbus_cfg));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()))
    assert got == [152, wm.Cfg.input_spectrum.offset, wm.Cfg.input_channels.offset, ctypes.sizeof(wm.ChannelHit), ctypes.sizeof(wm.Cfg)]
    assert ctypes.sizeof(wm.Timing) == 152 and wm.Cfg.input_channels.offset == wm.Cfg.input_spectrum.offset + 4


# ---- the restatement against a floating-point FFT ---------------------------------------------------------------------------------

def test_restatement_against_numpy_fft(wm):
    """z of the restatement against numpy.fft.fft of the same y (double), on the first 16 level blocks of the wideband fixture and on 16
    blocks of full-range random cs16.  The bound, per block and for every bin, on |z - X| as a complex number:
      - a twiddle multiply rounds each component once, by at most 1/2: sqrt(1/2) per multiply.  An output is a sum over the 2^(9 - s)
        stage-s values it is made of, each carrying one such rounding, s = 1 .. 9, and every later twiddle has magnitude 1 (to 2^-14.5):
        sqrt(1/2) (256 + 128 + ... + 1) = 361.4 at the very most;
      - a table entry is rint(16384 cos), rint(16384 sin): off by at most 1/2 per component, sqrt(1/2) / 16384 = 2^-14.5 of the twiddle.
        Nine stages, each acting on values whose magnitudes add up to sum |y| at most: 9 x 2^-14.5 x sum |y|.
    Both terms are worst cases (every rounding aligned); nothing in them comes from the code under test.
    Measured: wideband fixture, largest |z - X| 14.2 against a largest |X| of 24 013 (smallest bound of a block 411); full-range random
    cs16 58.0 against 1 069 047 (2730)."""
    raw, _ = CF.wideband(wm)
    rng = np.random.default_rng(2)
    for name, data, fmt in (("wideband", raw[:16 * PR.N * 4], FR.CS16), ("random", rng.integers(0, 256, 16 * PR.N * 4, dtype=np.uint8), FR.CS16)):
        y = PR.windowed(data, fmt)
        z = PR.dft(y)
        X = np.fft.fft(y[..., 0] + 1j * y[..., 1], axis=1)
        err = np.abs(z[..., 0] + 1j * z[..., 1] - X).max(axis=1)
        l1 = np.abs(y[..., 0] + 1j * y[..., 1]).sum(axis=1)
        bound = np.sqrt(0.5) * 511 + 9 * 2.0 ** -14.5 * l1
        print(f"{name}: largest |z - X| {err.max():.1f}, largest |X| {np.abs(X).max():.0f}, smallest bound {bound.min():.0f}")
        assert np.all(err <= bound), name


# ---- the device source on the block emulator ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h"), os.path.join(CSRC, "wm_k0_spectrum.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_spec_new.restype = ctypes.c_void_p
    L.wm_emu_spec_new.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
    L.wm_emu_spec_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_spec_preset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.wm_emu_spec_push.restype = ctypes.c_long
    L.wm_emu_spec_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.wm_emu_spec_read.restype = ctypes.c_long
    L.wm_emu_spec_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    return L


def run_emulated(emu, wm, raw, fmt, R, cuts, run, preset=None):
    """(sum, peak, blocks) after the pushes `cuts` (bytes) of raw, a wave taking `run` level blocks."""
    table = wm.shift_design(FS, 0)[1]
    h = emu.wm_emu_spec_new(fmt, table.ctypes.data, R, run)
    try:
        if preset is not None:
            emu.wm_emu_spec_preset(h, preset[0].ctypes.data, preset[1].ctypes.data, preset[2])
        off = 0
        for n in cuts:
            part = np.ascontiguousarray(raw[off:off + n]); off += n
            assert emu.wm_emu_spec_push(h, part.ctypes.data, part.size) == n // FR.BPS[fmt] // PR.N
        assert off == raw.size
        total, peak, blocks = np.zeros(PR.N, np.uint64), np.zeros(PR.N, np.uint32), ctypes.c_uint64()
        assert emu.wm_emu_spec_read(h, total.ctypes.data, peak.ctypes.data, ctypes.byref(blocks), 0) == PR.N
        return total, peak, int(blocks.value)
    finally:
        emu.wm_emu_spec_free(h)


def full_scale_inputs(fmt):
    """Four level blocks each: every sample at the format's negative full scale (cs16 all -32768: the largest pw, just above 2^31, and the
    largest |z|, just above 2^23 per component, in bin 256); a full-scale complex tone on the centre of bin 256 + 37; the same tone in I alone (a real
    tone: bins 256 +- 37)."""
    n = 4 * PR.N
    w = 2.0 * np.pi * 37 * np.arange(n) / PR.N
    tone = np.stack([np.cos(w), np.sin(w)], axis=1).reshape(-1)
    real = np.stack([np.cos(w), np.zeros(n)], axis=1).reshape(-1)
    if fmt == FR.CU8:
        q = lambda v: np.clip(np.rint(127.5 + 127.5 * v), 0, 255)
        lowest = np.zeros(2 * n)
    elif fmt == FR.CS8:
        q = lambda v: np.clip(np.rint(-0.5 + 127.5 * v), -128, 127)
        lowest = np.full(2 * n, -128)
    elif fmt == FR.CS16:
        q = lambda v: np.clip(np.rint(32767.5 * v - 0.5), -32768, 32767)
        lowest = np.full(2 * n, -32768)
    else:
        q = lambda v: v.astype(np.float32)
        lowest = np.full(2 * n, -1.0, np.float32)
    return {"lowest": FR.raw_bytes(lowest, fmt), "tone": FR.raw_bytes(q(tone), fmt), "real-tone": FR.raw_bytes(q(real), fmt)}


def named_inputs(fmt):
    rng = np.random.default_rng(0x5EC + fmt)
    n = N_BLOCKS * BLK
    zero = {FR.CU8: 128, FR.CS8: 0, FR.CS16: 0, FR.CF32: 0}[fmt]
    return dict(random=rng.integers(0, 256, n, dtype=np.uint8), zero=np.full(n, zero, np.uint8), **full_scale_inputs(fmt))


@pytest.mark.parametrize("R", [0, 6], ids=["R0", "R6"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fmt, R):
    """Random bit patterns (NaN and infinities among the cf32 ones), silence and the full-scale inputs, in one push with runs of 4;
    the random input also under every cut and with runs that do not divide a push (3, 5) and one longer than the pushes (16)."""
    for name, raw in named_inputs(fmt).items():
        want = PR.spectrum(raw, fmt, R)
        got = run_emulated(emu, wm, raw, fmt, R, [raw.size], 4)
        assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), name
        if name == "zero" and fmt in (FR.CS16, FR.CF32):         # (silence is x = 1 in the 8-bit formats: a little DC)
            assert not want[0].any() and not want[1].any()
        if name == "lowest" and not R:
            assert int(want[1].argmax()) == 256
            if fmt in (FR.CS16, FR.CF32):
                zc = 2 * int(PR.window().sum())                   # y = -2 w exactly, z = -2 sum w in both components: the largest pw there is
                assert int(want[1].max()) == (2 * zc * zc) >> 16 and 1 << 31 <= int(want[1].max()) < 1 << 32 and zc < 1 << 24
        if name != "random":
            continue
        assert want[2] == N_BLOCKS * BLK // FR.BPS[fmt] // PR.N
        for cut, run in (("one", 3), ("uneven", 5), ("uneven", 4), ("each-4096", 16), ("each-4096", 1)):
            got = run_emulated(emu, wm, raw, fmt, R, CUTS[cut], run)
            assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (cut, run)


def test_full_scale_tone_is_where_it_belongs(wm):
    """The restatement on the tone of full_scale_inputs: bin 256 + 37 holds it, the Hann window's two neighbours a quarter of its power,
    everything further away nothing worth mentioning -- the bin order and the sign of the frequency axis (f_b = (b - 256) Fin / 512)."""
    total, peak, blocks = PR.spectrum(full_scale_inputs(FR.CS16)["tone"], FR.CS16)
    b = int(peak.argmax())
    assert b == 256 + 37 and blocks == 4
    assert abs(int(peak[b - 1]) * 4 - int(peak[b])) < int(peak[b]) // 100 and abs(int(peak[b + 1]) * 4 - int(peak[b])) < int(peak[b]) // 100
    assert np.delete(peak, [b - 1, b, b + 1]).max() < int(peak[b]) >> 20
    assert 1 << 29 < int(peak[b]) <= 1 << 31


def test_accumulators_carry_in_64_bits_and_know_no_sample_counter(emu, wm):
    """K0SpecArgs holds no sample counter -- the kernel sees a push's level blocks, nothing of the stream's position -- so a stream beyond
    2^32 samples is a context whose accumulators already hold more than 2^23 level blocks.  Preset them beyond every 32-bit edge: the
    sums and the block count carry into their high words, the maxima stay maxima."""
    raw = np.random.default_rng(77).integers(0, 256, 8 * BLK, dtype=np.uint8)
    total, peak, blocks = PR.spectrum(raw, FR.CS16)
    rng = np.random.default_rng(78)
    pre = ((np.uint64(0xFFFFFFFF) - rng.integers(0, 1 << 20, PR.N).astype(np.uint64)), rng.integers(0, 1 << 32, PR.N, dtype=np.uint64).astype(np.uint32),
           (1 << 32) - 3)
    assert pre[2] * PR.N > 1 << 32 and blocks > 3
    got = run_emulated(emu, wm, raw, FR.CS16, 0, [3 * BLK, 5 * BLK], 3, preset=pre)
    assert got[2] == pre[2] + blocks and got[2] > 1 << 32
    assert np.array_equal(got[0], pre[0] + total) and np.all(got[0] > np.uint64(0xFFFFFFFF))
    assert np.array_equal(got[1], np.maximum(pre[1], peak))
    assert (got[1] == peak).any() and (got[1] == pre[1]).any()


# ---- the channel rule, and what the survey is for ----------------------------------------------------------------------------------

def noise_cu8(sigma):
    return np.clip(np.rint(127.5 + np.random.default_rng(900 + sigma).normal(0.0, sigma, 2 * PR.N * 2000)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def surveys(wm, samples):
    """name -> (Fin, sum, peak, blocks, raw bytes): every capture the rule is held to, surveyed once by the restatement."""
    s2 = samples["samples2"]
    s2 = s2[:s2.size // BLK * BLK]
    out = {"samples2": (FS, *PR.spectrum(s2, FR.CU8), s2)}
    for f in MIXES:
        raw = SR.round_trip_cu8(s2, FS, f)
        out[f"samples2{f:+d}"] = (FS, *PR.spectrum(raw, FR.CU8), raw)
    wide = CF.wideband(wm)[0]
    out["wideband"] = (CF.WIDE_FS, *PR.spectrum(wide, FR.CS16), wide)
    for sg in NOISE_SIGMAS:
        raw = noise_cu8(sg)
        out[f"noise{sg}"] = (FS, *PR.spectrum(raw, FR.CU8), raw)
    return out


def test_channels_in_c_equal_the_restated_rule(wm, surveys):
    """wmbus_spectrum_channels through ctypes against tests/spectrum_ref.py on every survey, with the defaults and with other widths,
    thresholds and rel; cap smaller than the hits; the refusals."""
    n_hits = {}
    for name, (fin, total, peak, blocks, _) in surveys.items():
        for kw in (dict(), dict(width_hz=100000), dict(width_hz=50000, min_ratio_q8=257, rel=1000), dict(width_hz=1, min_ratio_q8=300, rel=64),
                   dict(width_hz=fin, min_ratio_q8=260), dict(min_ratio_q8=2048, rel=2)):
            want = PR.channels(fin, total, peak, blocks, **kw)
            assert wm.spectrum_channels(fin, total, peak, blocks, **kw) == want, (name, kw)
            n_hits[name, tuple(kw)] = len(want)
            for cap in (0, 1, 2):
                assert wm.spectrum_channels(fin, total, peak, blocks, cap=cap, **kw) == want[:cap], (name, kw, cap)
    assert max(n_hits.values()) >= 8 and n_hits["wideband", ()] == 3
    fin, total, peak, blocks, _ = surveys["wideband"]
    # a synthetic max-hold: flat floor, one window's worth of bins at the very edge of the band, a tie between two equal peaks
    flat = np.full(PR.N, 1000, np.uint32)
    edge = flat.copy(); edge[:20] = 50000; edge[-3:] = 4000000000
    tie = flat.copy(); tie[100:110] = 70000; tie[300:310] = 70000
    for pk in (flat, edge, tie, np.zeros(PR.N, np.uint32), np.full(PR.N, 0xFFFFFFFF, np.uint32)):
        sm = pk.astype(np.uint64) * np.uint64(3)
        want = PR.channels(FS, sm, pk, 7)
        assert wm.spectrum_channels(FS, sm, pk, 7) == want
    assert [h["offset_hz"] < 0 for h in PR.channels(FS, tie.astype(np.uint64), tie, 1)] == [True, False]      # the lowest b wins a tie
    L, out = wm.lib(), (wm.ChannelHit * 4)()
    args = lambda in_hz=FS, blk=blocks, ratio=0: (in_hz, total.ctypes.data, peak.ctypes.data, blk, 0, ratio, 0, out, 4)
    assert L.wmbus_spectrum_channels(*args()) == 3
    assert L.wmbus_spectrum_channels(*args(in_hz=799999)) == -1 and PR.channels(799999, total, peak, blocks) is None
    assert L.wmbus_spectrum_channels(*args(blk=0)) == -1 and PR.channels(fin, total, peak, 0) is None
    for ratio in (1, 256):
        assert L.wmbus_spectrum_channels(*args(ratio=ratio)) == -1 and PR.channels(fin, total, peak, blocks, min_ratio_q8=ratio) is None
    assert L.wmbus_spectrum_channels(*args(ratio=257)) >= 3


def fields(text):
    return [ln.split(";") for ln in text.splitlines()]


@pytest.mark.parametrize("f", MIXES, ids=[f"{f:+d}" for f in MIXES])
def test_survey_then_decode_recovers_a_capture_tuned_off_its_channel(wm, oracle, surveys, f):
    """The bundled capture mixed by f (shift_ref.round_trip_cu8): undecodable as it stands; the survey reports exactly one transmitter,
    within 2 bins (Fin / 256) of where the unmixed capture's own hit plus f lies; decoding at the survey's offset gives the golden's four
    lines back, the first two with the golden's identity and payload, and at least three of them CRC-clean -- the golden has two: the
    survey also removes the dongle's own -10 kHz, which nobody had been told about.
    Measured (hit, error in bins of 3125 Hz, CRC fields): +200000: 189719, 0.00, 1,1,1,1; -43000: -53674, 0.12, 1,1,1,1; +60000: 49434,
    0.09, 1,1,1,1; -30000: -43118, 0.90, 1,1,0,1."""
    golden = fields(BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"])
    assert [g[2] for g in golden] == ["1", "1", "0", "0"]
    own = PR.channels(*surveys["samples2"][:4])
    assert len(own) == 1 and own[0]["offset_hz"] == -10290       # the dongle's own error
    fin, total, peak, blocks, raw = surveys[f"samples2{f:+d}"]
    opts = oracle.make_opts()
    assert oracle.run(raw, opts)["text"] == ""
    hits = PR.channels(fin, total, peak, blocks)
    assert len(hits) == 1
    hz = hits[0]["offset_hz"]
    err_bins = abs(hz - (own[0]["offset_hz"] + f)) / (FS / PR.N)
    got = fields(oracle.run(SR.pipeline_bytes(raw, FR.CU8, FS, hz, SR.CU8_ROUND_TRIP_GAIN), opts)["text"])
    print(f"{f:+d}: hit {hz} Hz x{hits[0]['ratio_q8'] / 256:.1f}, {err_bins:.2f} bins from the unmixed hit + f; CRC fields {','.join(g[2] for g in got)}")
    assert err_bins <= 2.0
    assert len(got) == 4
    assert [g[7:9] for g in got[:2]] == [g[7:9] for g in golden[:2]]
    assert sum(g[2] == "1" for g in got) >= 3


def test_wideband_fixture_gives_its_three_channels(surveys):
    """Exactly three hits, each within one bin (7812.5 Hz) of a channel of the fixture.  Measured: +698486, -602400, +453 Hz."""
    fin, total, peak, blocks, _ = surveys["wideband"]
    hits = PR.channels(fin, total, peak, blocks)
    print([h["offset_hz"] for h in hits])
    assert len(hits) == 3
    assert sorted(h["offset_hz"] for h in hits) == sorted(h["offset_hz"] for h in hits if min(abs(h["offset_hz"] - w) for w in CF.WIDE_HZ) <= fin / PR.N)
    for w in CF.WIDE_HZ:
        assert sum(abs(h["offset_hz"] - w) <= fin / PR.N for h in hits) == 1, w


@pytest.mark.parametrize("sigma", NOISE_SIGMAS)
def test_noise_alone_gives_no_channel(surveys, sigma):
    """cu8 noise, 2000 level blocks: nothing is reported; the strongest window stands x 1.1 over the floor against the threshold's x 4.
    Measured: B 256 / (W Fp) = 275, 274, 274, 270 for sigma 1, 3, 10, 30."""
    fin, total, peak, blocks, _ = surveys[f"noise{sigma}"]
    ratio = PR.strongest_ratio_q8(fin, peak)
    print(f"sigma {sigma}: strongest window {ratio} / 256 of the floor")
    assert PR.channels(fin, total, peak, blocks) == [] and ratio < PR.MIN_RATIO_Q8
