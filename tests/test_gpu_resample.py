"""cfg.input_rate_hz on the GPU: the resampler kernel's bytes against the numpy restatement (tests/resample_ref.py), the datagram
text against the oracle on the restated bytes (single context, wmbus_batch, CLI), the yield against a native capture, and a
real recording brought to 2.048 MS/s and back."""
import json
import os
import subprocess

import numpy as np
import pytest

import resample_ref as RR
from lanes import one_lane
from test_resample_emulated import BLK, CUTS, IDS, N_BLOCKS, N_YIELD, RATES, WORST, WORST_IDS, crc_clean, received, worst_yield_captures, yield_captures

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = 1 | 2 | 4 | 8                                 # T1 + C1 (both frame formats) + S1
# synthetic captures at the raw rate: (generator fs_khz, decimation)
TEXT_RATES = [(2048, 2), (2000, 2), (2560, 2), (1000, 1)]


def push_all(rx, streams, cuts):
    """Raw pushes through a Receiver; returns (per stream: resampled bytes handed to the pipeline, text)."""
    got = [[] for _ in streams]
    text = [[] for _ in streams]
    off = 0
    for n in cuts:
        rx.push([a[off:off + n] for a in streams]); off += n
        for s in range(len(streams)):
            got[s].append(rx.read_resampled(s))
        for ln in rx.lines():
            text[ln["stream"]].append(ln["text"])
    return [np.concatenate(g) for g in got], ["".join(t) for t in text]


@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven"])
@pytest.mark.parametrize("n_streams", [1, 8])
@pytest.mark.parametrize("fin,d", RATES, ids=IDS)
def test_resampled_bytes_equal_the_restatement(wm, fin, d, n_streams, cut, windows):
    L, M, T, taps = wm.resampler_design(fin, 800000 * d)
    rng = np.random.default_rng(fin + n_streams)
    caps = [rng.integers(0, 256, N_BLOCKS * BLK, dtype=np.uint8) for _ in range(n_streams)]
    if n_streams > 1:
        caps[1][:] = 0; caps[2][:] = 255
        caps[3][:] = np.repeat(np.where((np.arange(caps[3].size // 2) // (3 * T)) % 2 == 0, 0, 255).astype(np.uint8), 2)
    with wm.Receiver(n_streams=n_streams, max_push_bytes=N_BLOCKS * BLK, decimation=d, input_rate_hz=fin, input_windows=windows) as rx:
        got, _ = push_all(rx, caps, CUTS[cut])
        assert rx.resampler_launches() == len(CUTS[cut])
    for s in range(n_streams):
        want = RR.pipeline_bytes(caps[s], L, M, taps)
        assert got[s].size == want.size, s
        assert np.array_equal(got[s], want), (s, int(np.argmax(got[s] != want)))


def test_a_push_that_completes_no_block_yields_no_lines(wm):
    """10 MS/s -> 1.6 MS/s: 4096 raw bytes are 655 or 656 resampled ones; the pipeline gets a block with every sixth or seventh push."""
    fin = 10000000
    L, M, T, taps = wm.resampler_design(fin, 1600000)
    cu8 = np.random.default_rng(7).integers(0, 256, 30 * BLK, dtype=np.uint8)
    with wm.Receiver(n_streams=1, max_push_bytes=BLK, input_rate_hz=fin) as rx:
        sizes, got = [], []
        for k in range(30):
            rx.push([cu8[k * BLK:(k + 1) * BLK]])
            got.append(rx.read_resampled(0)); sizes.append(got[-1].size)
            if sizes[-1] == 0:
                assert rx.lines() == []
    assert set(sizes) == {0, BLK} and sizes.count(BLK) == RR.resample(cu8, L, M, taps).size // BLK
    assert np.array_equal(np.concatenate(got), RR.pipeline_bytes(cu8, L, M, taps))


def test_without_a_rate_no_resampler_kernel_is_launched(wm, oracle):
    cu8 = wm.synth_capture(seed=11, n_samples=1 << 18, kinds=KINDS, frames_per_s=60.0)[0]
    want = oracle.run(cu8, oracle.make_opts())["text"]
    for rate in (0, 1600000):                           # the native rate is the same as no rate
        with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, input_rate_hz=rate) as rx:
            assert rx.run(cu8)[0] == want
            assert rx.resampler_launches() == 0
            with pytest.raises(wm.WmbusError):
                rx.read_resampled(0)


def test_bad_rates_are_refused_at_open(wm):
    for rate, d in ((700000, 2), (2047999, 2), (40000000, 1)):
        with pytest.raises(wm.WmbusError, match="input_rate_hz"):
            wm.Receiver(n_streams=1, max_push_bytes=1 << 16, decimation=d, input_rate_hz=rate)
    with pytest.raises(wm.WmbusError, match="polyphase"):      # -P is the 1.6 MS/s design whatever the input rate
        wm.Receiver(n_streams=1, max_push_bytes=1 << 16, decimation=3, prefilter=1, input_rate_hz=2048000)


def synth_at(wm, fs_khz, seed, n_samples=1 << 20, **kw):
    return wm.synth_capture(seed=seed, n_samples=n_samples, fs_khz=fs_khz, kinds=KINDS, frames_per_s=60.0, **kw)


@pytest.mark.parametrize("fs_khz,d", TEXT_RATES, ids=[str(r[0]) for r in TEXT_RATES])
def test_text_equals_the_oracle_on_the_restated_bytes(wm, oracle, fs_khz, d):
    caps, want = text_captures(wm, oracle, fs_khz, d)
    # single context: one push, and ragged pushes through both input windows
    with wm.Receiver(n_streams=3, max_push_bytes=caps[0].size, decimation=d, input_rate_hz=fs_khz * 1000) as rx:
        assert rx.run(caps) == want
    with wm.Receiver(n_streams=3, max_push_bytes=1 << 19, decimation=d, input_rate_hz=fs_khz * 1000, input_windows=2, keep_taps=False) as rx:
        assert rx.run(caps, push_bytes=BLK * 97) == want
    # wmbus_batch, host-sourced
    push = 1 << 19
    text = [""] * 3
    with wm.Batch(n_streams=3, max_push_bytes=push, decimation=d, input_rate_hz=fs_khz * 1000, input_windows=2) as b:
        pos = {}

        def fill(first, n, slab):
            off = pos.get(first, 0)
            k = min(push, caps[0].size - off)
            for s in range(n):
                slab[s, :k] = caps[first + s][off:off + k]
            pos[first] = off + k
            return k

        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        st = b.run_from(fill, on_push)
        assert st["samples"] == 3 * caps[0].size // 2         # raw samples consumed
    assert text == want


_TEXT = {}


def text_captures(wm, oracle, fs_khz, d, n_samples=1 << 20, seed=7100, long_=False):
    """Three captures at a raw rate and the oracle's text on the restated bytes: computed once per rate, shared, left unchanged."""
    key = (fs_khz, d, seed)
    if key not in _TEXT:
        L, M, T, taps = wm.resampler_design(fs_khz * 1000, 800000 * d)
        caps = [synth_at(wm, fs_khz, seed + fs_khz + s, n_samples=n_samples)[0] for s in range(3)]
        want = []
        for c in caps:
            y = RR.resample_long(c, L, M, taps) if long_ else RR.pipeline_bytes(c, L, M, taps)
            want.append(oracle.run(y[:y.size // BLK * BLK], oracle.make_opts(decimation=d))["text"])
            c.setflags(write=False)
        assert all(len(w.splitlines()) >= 10 for w in want)
        _TEXT[key] = (caps, want)
    return _TEXT[key]


def lane_leg(wm, caps, want, push, d, fs_khz):
    """A batch case as two contexts of two captures in ONE lane (the fourth capture is the first again): the resampler recorded and
    issued behind the mate's operations, several pushes."""
    sizes = [min(push, caps[0].size - off) for off in range(0, caps[0].size, push)]
    assert len(sizes) >= 2
    got = one_lane(wm, caps + [caps[0]], 4, push=push, sizes_of={0: sizes, 2: sizes}, decimation=d, input_rate_hz=fs_khz * 1000, input_windows=2)
    assert got.plan == [(0, 2), (2, 2)] and got.run_stats["samples"] == 4 * caps[0].size // 2
    assert [got.whole_text(s) for s in range(4)] == want + [want[0]]


@pytest.mark.parametrize("fs_khz,d", TEXT_RATES, ids=[str(r[0]) for r in TEXT_RATES])
def test_text_in_one_lane(wm, oracle, fs_khz, d):
    caps, want = text_captures(wm, oracle, fs_khz, d)
    lane_leg(wm, caps, want, 1 << 19, d, fs_khz)


# (generator fs_khz, decimation, samples): upsampling 8 / 5 (T = 16) and 1 / 32 (T = 512)
CORNER_TEXT_RATES = [(1000, 2, 1 << 20), (25600, 1, 1 << 24)]


@pytest.mark.parametrize("fs_khz,d,n_samples", CORNER_TEXT_RATES, ids=[str(r[0]) for r in CORNER_TEXT_RATES])
def test_text_at_two_corner_rates_equals_the_oracle_on_the_restated_bytes(wm, oracle, fs_khz, d, n_samples):
    L, M, T, taps = wm.resampler_design(fs_khz * 1000, 800000 * d)
    assert L > M or T >= 256
    caps, want = text_captures(wm, oracle, fs_khz, d, n_samples=n_samples, seed=7300, long_=True)
    push = 1 << 21
    with wm.Receiver(n_streams=3, max_push_bytes=push, decimation=d, input_rate_hz=fs_khz * 1000, input_windows=2, keep_taps=False) as rx:
        assert rx.run(caps, push_bytes=BLK * 97) == want
    text = [""] * 3
    with wm.Batch(n_streams=3, max_push_bytes=push, decimation=d, input_rate_hz=fs_khz * 1000, input_windows=2) as b:
        pos = {}

        def fill(first, n, slab):
            off = pos.get(first, 0)
            k = min(push, caps[0].size - off)
            for s in range(n):
                slab[s, :k] = caps[first + s][off:off + k]
            pos[first] = off + k
            return k

        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        st = b.run_from(fill, on_push)
        assert st["samples"] == 3 * caps[0].size // 2
    assert text == want


@pytest.mark.parametrize("fs_khz,d,n_samples", CORNER_TEXT_RATES, ids=[str(r[0]) for r in CORNER_TEXT_RATES])
def test_text_at_two_corner_rates_in_one_lane(wm, oracle, fs_khz, d, n_samples):
    caps, want = text_captures(wm, oracle, fs_khz, d, n_samples=n_samples, seed=7300, long_=True)
    lane_leg(wm, caps, want, min(1 << 21, caps[0].size // 2), d, fs_khz)      # two pushes at least: a carry


@pytest.mark.parametrize("fin,d", WORST, ids=WORST_IDS)
def test_capture_at_the_worst_ratios_is_received_like_a_native_one_on_the_gpu(wm, oracle, fin, d):
    raw, fr_raw, nat, fr_nat = worst_yield_captures(wm, fin, d)
    with wm.Receiver(n_streams=1, max_push_bytes=4 << 20, decimation=d, input_rate_hz=fin) as rx:
        got = received(fr_raw, rx.run(raw)[0])
    ref = received(fr_nat, oracle.run(nat, oracle.make_opts(decimation=d))["text"])
    print(f"{fin} -> {800000 * d}: of the first {N_YIELD} frames placed: received resampled (GPU) {got}, native (oracle) {ref}")
    assert got >= ref - 0.02 * N_YIELD


def test_simultaneous_reception_behind_the_resampler(wm, oracle):
    """-s: 2.56 MS/s -> 1.6 MS/s with the generator's +-325 kHz layout."""
    L, M, T, taps = wm.resampler_design(2560000, 1600000)
    cu8 = synth_at(wm, 2560, 9090, t1c1_center_khz=325.0, s1_center_khz=-325.0)[0]
    want = oracle.run(RR.pipeline_bytes(cu8, L, M, taps), oracle.make_opts(simultaneous=1))["text"]
    assert len(want.splitlines()) >= 10
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 19, simultaneous=True, input_rate_hz=2560000) as rx:
        assert rx.run(cu8)[0] == want


def test_resampled_capture_is_received_like_a_native_one_on_the_gpu(wm, oracle):
    raw, fr_raw, nat, fr_nat = yield_captures(wm)
    with wm.Receiver(n_streams=1, max_push_bytes=4 << 20, input_rate_hz=2048000) as rx:
        got = received(fr_raw, rx.run(raw)[0])
    ref = received(fr_nat, oracle.run(nat, oracle.make_opts())["text"])
    print(f"of the first {N_YIELD} frames placed: received resampled (GPU) {got}, native (oracle) {ref}")
    assert got >= ref - 0.02 * N_YIELD


def test_real_recording_round_trip(wm, samples):
    from scipy.signal import resample_poly
    want = crc_clean(json.load(open(os.path.join(HERE, "golden", "bundled.json")))["rtlsdr_868.950M_1M6_samples2.cu8|-v"])
    x = samples["samples2"].reshape(-1, 2).astype(np.float64) - 127.5
    raw = np.clip(np.rint(resample_poly(x, 32, 25, axis=0) + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 20, input_rate_hz=2048000) as rx:
        got = crc_clean(rx.run(raw)[0])
    assert len(want) >= 1 and want <= got, want - got


def test_cli_R(wm, oracle, tmp_path):
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    L, M, T, taps = wm.resampler_design(2048000, 1600000)
    caps = {"a.cu8": synth_at(wm, 2048, 9191)[0], "b.cu8": synth_at(wm, 2048, 9192, n_samples=3 << 18)[0]}
    want = {k: oracle.run(RR.pipeline_bytes(c, L, M, taps), oracle.make_opts())["text"] for k, c in caps.items()}
    for spelling in ("2.048M", "2048k", "2048000"):
        p = subprocess.run([wm.CLI_PATH, "-R", spelling, "-v", "-B", str(1 << 19)], input=caps["a.cu8"].tobytes(), capture_output=True, env=env)
        assert p.returncode == 0, p.stderr
        assert p.stdout.decode() == want["a.cu8"]
    # batch mode (-S) and -G all
    for name, c in caps.items():
        c.tofile(tmp_path / name)
    # the shorter file is padded with mid-scale bytes to the longer one's length: the same as decoding it followed by silence
    pad = np.concatenate([caps["b.cu8"], np.full(caps["a.cu8"].size - caps["b.cu8"].size, 128, np.uint8)])
    want["b.cu8"] = oracle.run(RR.pipeline_bytes(pad, L, M, taps), oracle.make_opts())["text"]
    for extra in (["-S"], ["-G", "all"]):
        p = subprocess.run([wm.CLI_PATH, "-R", "2.048M", "-v", "-B", str(1 << 19)] + extra + list(caps), cwd=tmp_path, capture_output=True, env=env)
        assert p.returncode == 0, p.stderr
        got = {name: "" for name in caps}
        for line in p.stdout.decode().splitlines(True):
            name, rest = line.split(": ", 1)
            got[name] += rest
        assert got == want, extra
    for bad in ("abc", "0", "2.0479995M", "100k", "2048000x"):
        p = subprocess.run([wm.CLI_PATH, "-R", bad], input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode(), bad
    p = subprocess.run([wm.CLI_PATH, "-R", "2.048M", "-P", "-d", "4"], input=b"", capture_output=True, env=env)
    assert p.returncode == 1 and b"polyphase" in p.stderr
