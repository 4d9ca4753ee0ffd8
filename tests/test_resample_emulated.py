"""k0_resample (device source rtl-wmbus_amd/csrc/wm_k0_resample.h) on the coroutine block emulator against the numpy
restatement tests/resample_ref.py, byte for byte; and the filter's quality: what the oracle receives from a resampled capture
against what it receives from the same traffic generated at the native rate.  No GPU needed."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import resample_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtl-wmbus_amd", "csrc")
SO = os.path.join(HERE, "emu", "libresample_emu.so")
SRC = os.path.join(HERE, "emu", "resample_emu.cpp")
BLK = 4096

RATES = [(2048000, 2), (2000000, 2), (2400000, 2), (2560000, 2), (3000000, 2), (1000000, 1), (10000000, 2)]
IDS = [f"{r[0]}-d{r[1]}" for r in RATES]
N_BLOCKS = 21                                       # 3 + 1 + 17: the uneven cut below covers the input exactly
CUTS = {"each-4096": [BLK] * N_BLOCKS, "uneven": [BLK * 3, BLK, BLK * 17], "one": [BLK * N_BLOCKS]}


@pytest.fixture(scope="module")
def emu():
    deps = [SRC, os.path.join(HERE, "emu", "block_emu.h"), os.path.join(CSRC, "wm_k0_resample.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(HERE, "emu"),
                        "-Wno-unknown-pragmas", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.wm_emu_k0_new.restype = ctypes.c_void_p
    L.wm_emu_k0_new.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    L.wm_emu_k0_free.argtypes = [ctypes.c_void_p]
    L.wm_emu_k0_push.restype = ctypes.c_long
    L.wm_emu_k0_push.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    L.wm_emu_k0_pick_tile.restype = ctypes.c_uint
    L.wm_emu_k0_pick_tile.argtypes = [ctypes.c_uint] * 3
    L.wm_emu_k0_lds_bytes.restype = ctypes.c_uint
    L.wm_emu_k0_lds_bytes.argtypes = [ctypes.c_uint] * 4
    L.wm_emu_k0_span.restype = ctypes.c_uint
    L.wm_emu_k0_span.argtypes = [ctypes.c_uint] * 4
    L.wm_emu_k0_start_at.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    return L


def library_tile(emu, L, M, T):
    """The tile wmbus_open picks (k0_pick_tile): whole groups of 4 L outputs, LDS at most 64 KiB."""
    tile = emu.wm_emu_k0_pick_tile(L, M, T)
    assert tile > 0 and tile % (4 * L) == 0 and emu.wm_emu_k0_lds_bytes(L, M, T, tile) <= 65536
    return tile


def run_emulated(emu, cu8, L, M, taps, cuts, tile):
    """The bytes the pipeline takes, push by push, concatenated."""
    T = taps.shape[1]
    taps = np.ascontiguousarray(taps, np.int16)
    h = emu.wm_emu_k0_new(L, M, T, taps.ctypes.data, tile)
    got, off = [], 0
    try:
        for n in cuts:
            raw = np.ascontiguousarray(cu8[off:off + n]); off += n
            win = np.full(BLK + 2 * RR.n_outputs(n // 2, L, M) + 64, 0xA5, np.uint8)
            r = emu.wm_emu_k0_push(h, raw.ctypes.data, raw.size, win.ctypes.data, win.size - 64)
            assert r >= 0 and r % BLK == 0
            assert np.all(win[-64:] == 0xA5)                 # nothing written past the window
            got.append(win[:r].copy())
    finally:
        emu.wm_emu_k0_free(h)
    assert off == cu8.size
    return np.concatenate(got)


def inputs(n_bytes, T=32):
    rng = np.random.default_rng(0x5EED)
    sq = np.where((np.arange(n_bytes // 2) // (3 * T)) % 2 == 0, 0, 255).astype(np.uint8)      # full scale, well inside the pass band: the overshoot at its edges clamps
    return {"random": rng.integers(0, 256, n_bytes, dtype=np.uint8), "zeros": np.zeros(n_bytes, np.uint8),
            "ones": np.full(n_bytes, 255, np.uint8), "square": np.repeat(sq, 2)}


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("fin,d", RATES, ids=IDS)
def test_device_source_on_host_matches_the_restatement(emu, wm, fin, d, cut):
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    tile = library_tile(emu, L, M, T)
    for name, cu8 in inputs(N_BLOCKS * BLK, T).items():
        want = RR.pipeline_bytes(cu8, L, M, taps)
        got = run_emulated(emu, cu8, L, M, taps, CUTS[cut], tile)
        assert got.size == want.size, name
        assert np.array_equal(got, want), (name, int(np.argmax(got != want)))
        if name == "square":
            assert want.min() == 0 and want.max() == 255      # the clamp is reached
        if name == "zeros":
            assert np.all(want[2 * T:] == 0)
        if name == "ones":
            assert np.all(want[2 * T:] == 255)


@pytest.mark.parametrize("fin,d", [(2048000, 2), (10000000, 2), (1000000, 2)], ids=["2048000", "10000000", "1000000-up"])
def test_result_does_not_depend_on_the_tile(emu, wm, fin, d):
    """Small tiles: many blocks per push, block edges at every phase (1 MS/s -> 1.6 MS/s also covers L > M)."""
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    cu8 = inputs(N_BLOCKS * BLK)["random"]
    want = RR.pipeline_bytes(cu8, L, M, taps)
    for tile in (64, 190):
        assert np.array_equal(run_emulated(emu, cu8, L, M, taps, CUTS["uneven"], tile), want), tile


SMALL_TILE = 190                                    # not a multiple of any 4 L: every block ends in a partial group


def design_inputs(n_bytes, T):
    named = inputs(n_bytes, T)
    return {"random": named["random"], "min": named["zeros"], "max": named["ones"], "square": named["square"]}


FULL = os.environ.get("WMBUS_RESAMPLE_FULL") == "1"


def check_design_on_the_emulator(emu, wm, fin, d, full=True):
    """One design, cu8 at gain x 1 through the kernel's cu8 entry point: the library's tile under all three cuts, the small odd tile
    under the uneven one, four inputs, the input sized so that the pipeline gets at least three whole blocks.  full=False (the drawn
    designs, unless WMBUS_RESAMPLE_FULL=1): random and square only, 4096-byte pushes with the library's tile, the uneven cut with
    the small one."""
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    assert (L, M, T) == RR.geometry(fin, d)
    tile = library_tile(emu, L, M, T)
    n_bytes = RR.blocks_input(L, M, 2)
    cuts = RR.cuts_for(n_bytes)
    for name, cu8 in design_inputs(n_bytes, T).items():
        if not full and name not in ("random", "square"):
            continue
        want = RR.pipeline_bytes(cu8, L, M, taps)
        assert want.size // BLK >= 3
        for cut, tl in ([("one", tile), ("uneven", tile)] if full else []) + [("each-4096", tile), ("uneven", SMALL_TILE)]:
            got = run_emulated(emu, cu8, L, M, taps, cuts[cut], tl)
            assert got.size == want.size, (name, cut, tl)
            assert np.array_equal(got, want), (name, cut, tl, int(np.argmax(got != want)))
        if name == "square":
            assert want.min() == 0 and want.max() == 255      # the clamp is reached
        if name == "min":
            assert np.all(want[2 * T * max(1, L // M + 1):] == 0)
        if name == "max":
            assert np.all(want[2 * T * max(1, L // M + 1):] == 255)


@pytest.mark.parametrize("fin,d", RR.CORNERS, ids=RR.CORNER_IDS)
def test_corners_on_host_match_the_restatement(emu, wm, fin, d):
    check_design_on_the_emulator(emu, wm, fin, d)


def test_sampled_designs_on_host_match_the_restatement(emu, wm):
    """The seeded draw of tests/resample_ref.py::sample_designs (WMBUS_RESAMPLE_N, WMBUS_RESAMPLE_SEED): with the corners, every value
    of T and every value of L that the library accepts."""
    for fin, d in RR.sample_designs():
        check_design_on_the_emulator(emu, wm, fin, d, full=FULL)


def test_long_restatement_equals_the_plain_one(wm):
    rng = np.random.default_rng(3)
    for fin, d in [(25600000, 1), (3200000, 2), (1000000, 2), (2048000, 2), (25575000, 1)]:
        L, M, T, taps = wm.resampler_design(fin, 800000 * d)
        cu8 = rng.integers(0, 256, 2 * (3000 * M // L + 777), dtype=np.uint8)
        assert np.array_equal(RR.resample_long(cu8, L, M, taps, chunk=1000), RR.resample(cu8, L, M, taps)), (fin, d)


def crc_clean(text):
    return {l.split(";")[-1][2:] for l in text.splitlines() if l.split(";")[2] == "1"}


def received(frames, text):
    good = crc_clean(text)
    return sum(1 for f in frames if f["complete"] and f["telegram"].hex() in good)


N_YIELD = 300                                       # frames compared; 2 % of them is six frames


def yield_captures(wm):
    """The 2.048 MS/s capture and its native twin: same seed, same traffic settings, 6.5 s each.  The generator draws its noise
    from the same random sequence as its traffic, so the two captures hold DIFFERENT frames (353 and 362 of them with this seed):
    an absolute count over whole captures would compare how many frames each happened to place.  Both yields are therefore
    counted over the first N_YIELD frames placed, which makes 'frames placed' the same number on both sides."""
    seed, seconds, kinds = 0xA11CE, 6.5, wm.T1 | wm.C1A | wm.C1B | wm.S1
    raw, fr_raw = wm.synth_capture(seed=seed, n_samples=int(2048000 * seconds) // 2048 * 2048, fs_khz=2048, kinds=kinds, frames_per_s=160.0)
    nat, fr_nat = wm.synth_capture(seed=seed, n_samples=int(1600000 * seconds) // 2048 * 2048, fs_khz=1600, kinds=kinds, frames_per_s=160.0)
    assert len(fr_raw) >= N_YIELD and len(fr_nat) >= N_YIELD
    return raw, fr_raw[:N_YIELD], nat, fr_nat[:N_YIELD]


def test_resampled_capture_is_received_like_a_native_one(wm, oracle):
    """2.048 MS/s synthetic traffic through the restated resampler and the oracle, against the same seed generated at 1.6 MS/s and
    decoded by the oracle alone (the reference's own yield): at least the native yield minus 2 % of the frames placed."""
    raw, fr_raw, nat, fr_nat = yield_captures(wm)
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    opts = oracle.make_opts()
    got = received(fr_raw, oracle.run(RR.pipeline_bytes(raw, L, M, taps), opts)["text"])
    ref = received(fr_nat, oracle.run(nat, opts)["text"])
    print(f"of the first {N_YIELD} frames placed: received resampled {got}, native {ref}")
    assert got >= ref - 0.02 * N_YIELD


# The designs the response test ranks worst (tests/test_resampler_design.py::test_response_against_the_float_design): the integer
# ratio 1 / 2 (float design already at -57.9 dB: no slack in T) and the T = 512 ratio 1 / 32 (Q14 rounding floor): (in_hz, decimation)
WORST = [(3200000, 2), (25600000, 1)]
WORST_IDS = [f"{f}-d{d}" for f, d in WORST]


def worst_yield_captures(wm, fin, d):
    """yield_captures() at another rate: same seed, same traffic, 6.5 s, the native twin at decimation x 800 kHz.  The generator
    places about 55 frames a second with these settings, so N_YIELD frames need nearly the whole 6.5 s at any rate: nothing is
    shortened."""
    assert fin % 1000 == 0
    seed, seconds, kinds = 0xA11CE, 6.5, wm.T1 | wm.C1A | wm.C1B | wm.S1
    raw, fr_raw = wm.synth_capture(seed=seed, n_samples=int(fin * seconds) // 2048 * 2048, fs_khz=fin // 1000, kinds=kinds, frames_per_s=160.0)
    nat, fr_nat = wm.synth_capture(seed=seed, n_samples=int(800000 * d * seconds) // 2048 * 2048, fs_khz=800 * d, kinds=kinds, frames_per_s=160.0)
    assert len(fr_raw) >= N_YIELD and len(fr_nat) >= N_YIELD
    return raw, fr_raw[:N_YIELD], nat, fr_nat[:N_YIELD]


@pytest.mark.parametrize("fin,d", WORST, ids=WORST_IDS)
def test_capture_at_the_worst_ratios_is_received_like_a_native_one(wm, oracle, fin, d):
    """test_resampled_capture_is_received_like_a_native_one at the ratios with the poorest stop band: the same reference (the oracle
    on the native twin) and the same margin."""
    raw, fr_raw, nat, fr_nat = worst_yield_captures(wm, fin, d)
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    opts = oracle.make_opts(decimation=d)
    y = RR.resample_long(raw, L, M, taps)
    got = received(fr_raw, oracle.run(y[:y.size // BLK * BLK], opts)["text"])
    ref = received(fr_nat, oracle.run(nat, opts)["text"])
    print(f"{fin} -> {800000 * d}: of the first {N_YIELD} frames placed: received resampled {got}, native {ref}")
    assert got >= ref - 0.02 * N_YIELD


def test_real_recording_round_trip_through_the_restatement(wm, oracle, samples):
    """The bundled 1.6 MS/s recording brought to 2.048 MS/s in float (scipy resample_poly 32 / 25, rounded to cu8), back through the
    restated resampler, decoded by the oracle: every distinct CRC-clean telegram of the recording's golden appears CRC-clean."""
    from scipy.signal import resample_poly
    golden = json.load(open(os.path.join(HERE, "golden", "bundled.json")))["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    want = crc_clean(golden)
    assert len(want) >= 1
    x = samples["samples2"].reshape(-1, 2).astype(np.float64) - 127.5
    up = resample_poly(x, 32, 25, axis=0)
    raw = np.clip(np.rint(up + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    raw = raw[:raw.size // BLK * BLK]
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    got = crc_clean(oracle.run(RR.pipeline_bytes(raw, L, M, taps), oracle.make_opts())["text"])
    assert want <= got, want - got
