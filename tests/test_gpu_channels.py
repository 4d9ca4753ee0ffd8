"""cfg.input_channels on the GPU: several channels of one wideband capture in one context.  The bytes of every pipeline stream against
the single-shift restatement (tests/shift_ref.py, dc_ref.py, agc_ref.py) per channel; the contract itself, GPU against GPU -- lines,
level records and chips of channel c equal those of a single-shift context with input_shift_hz = hz[c]; the bundled 868.625 MHz capture
at +-325 kHz without -s; the blocker and the AGC per capture; a batch; the CLI's -O list; input_channels = 0 is the context it always
was; refusals."""
import json
import os
import subprocess

import numpy as np
import pytest

import channels_fixture as CF
import format_ref as FR
import shift_ref as SR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS
from test_resample_emulated import BLK, CUTS, N_BLOCKS
from test_shift_emulated import shift_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = json.load(open(os.path.join(HERE, "golden", "bundled.json")))
OUT_HZ = 1600000
RATES = [0, 2048000, 2500000]
LISTS = ["two", "edges"]
WIDE_KW = dict(input_rate_hz=CF.WIDE_FS, input_format=FR.CS16, input_gain_q8=CF.WIDE_GAIN)
SWAPPED_HZ = [CF.WIDE_HZ[1], CF.WIDE_HZ[0], CF.WIDE_HZ[2]]      # the second capture: the first with its first two channels swapped
GAIN_DB = "4.07"                                    # the CLI's spelling of gain 409: rint(256 * 10^(4.07 / 20)) = 409


def design(wm, rate):
    if rate == 0:
        return 1, 1, None
    L, M, T, taps = wm.resampler_design(rate, OUT_HZ)
    return L, M, taps


def channel_list(name, rate):
    fin = rate or OUT_HZ
    return {"two": [200000, -123457], "edges": [0, -(fin // 2), 1]}[name]


@pytest.fixture(scope="module")
def wide(wm, oracle):
    """The fixture tests/test_channels_emulated.py pins: raw bytes of two captures (the second with channels swapped), and per capture and
    channel the oracle's text on the restated bytes."""
    L, M, T, taps = wm.resampler_design(CF.WIDE_FS, OUT_HZ)
    caps = [CF.wideband(wm)[0], CF.wideband(wm, SWAPPED_HZ)[0]]
    text = [[oracle.run(np.ascontiguousarray(SR.pipeline_bytes(raw, FR.CS16, CF.WIDE_FS, f, CF.WIDE_GAIN, L, M, taps)), oracle.make_opts())["text"]
             for f in CF.WIDE_HZ] for raw in caps]
    assert all(len(t.splitlines()) >= 6 for t in text[0])
    return dict(caps=caps, text=text, taps=(L, M, taps))


# ---- 1. the bytes of every pipeline stream ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("windows", [1, 2])
@pytest.mark.parametrize("cut", ["one", "uneven"])
@pytest.mark.parametrize("n_cap", [1, 3])
@pytest.mark.parametrize("chans", LISTS)
@pytest.mark.parametrize("rate", RATES, ids=[str(r) if r else "native" for r in RATES])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_bytes_and_clip_count_equal_the_restatement_per_channel(wm, fmt, rate, chans, n_cap, cut, windows):
    """A different capture per stream, so that a v / C or a stride mix-up shows; gain x 1 on one capture, x 16 (random full-range input
    clips) on three.  read_resampled takes the pipeline stream v = capture * C + channel."""
    L, M, taps = design(wm, rate)
    fin, hz = rate or OUT_HZ, channel_list(chans, rate)
    C = len(hz)
    named = shift_inputs(fmt, N_BLOCKS * BLK)
    names = list(named)
    caps = [named[names[k]] for k in range(n_cap)]
    g = 256 if n_cap == 1 else 4096
    with wm.Receiver(n_streams=n_cap, max_push_bytes=N_BLOCKS * BLK, input_rate_hz=rate, input_channel_hz=hz, input_format=fmt, input_gain_q8=g,
                     input_windows=windows) as rx:
        got, off, clipped, bytes_out = [[] for _ in range(n_cap * C)], 0, 0, 0
        for n in CUTS[cut]:
            rx.push([a[off:off + n] for a in caps]); off += n
            for v in range(n_cap * C):
                got[v].append(rx.read_resampled(v))
            tm = rx.timing()
            clipped += tm["input_clipped"]; bytes_out += tm["input_bytes_out"]
        assert rx.resampler_launches() == len(CUTS[cut])
        with pytest.raises(wm.WmbusError):
            rx.read_resampled(n_cap * C)
    want_clips = want_bytes = 0
    for k in range(n_cap):
        for c, f in enumerate(hz):
            y, clips = SR.convert(caps[k], fmt, fin, f, g, L, M, taps)
            want = CF.whole_blocks(y)
            have = np.concatenate(got[k * C + c])
            assert have.size == want.size, (k, c)
            assert np.array_equal(have, want), (k, c, int(np.argmax(have != want)))
            want_clips += clips; want_bytes += y.size
    assert clipped == want_clips                             # summed over channels
    assert bytes_out == want_bytes


# ---- 2. the contract: channel c is the single-shift context ------------------------------------------------------------------------

def run_with_levels(rx, caps, push_bytes, width):
    """(text per pipeline stream, level records per pipeline stream, (stream, channel) of every line in order)."""
    text, levels, keys = [""] * width, [[] for _ in range(width)], []
    C = rx.n_channels
    total = caps[0].size // BLK * BLK
    for off in range(0, total, push_bytes):
        n = min(push_bytes, total - off)
        rx.push([a[off:off + n] for a in caps])
        lines, lev = rx.lines(), rx.line_levels()
        assert len(lev) == len(lines)
        for ln, lv in zip(lines, lev):
            v = ln["stream"] * C + ln["channel"]
            text[v] += ln["text"]; levels[v].append(lv); keys.append((ln["stream"], ln["channel"]))
    return text, levels, keys


@pytest.mark.parametrize("rounds_on_host", [False, True], ids=["rounds-on-gpu", "rounds-on-host"])
@pytest.mark.parametrize("push", [None, BLK * 37], ids=["one-push", "pushes-of-37-blocks"])
def test_channel_c_is_the_single_shift_context(wm, wide, push, rounds_on_host):
    """C = 3 on two 4.0 MS/s captures against three single-shift Receivers: equal lines, equal level records, equal chips; the lines are
    also the oracle's on the restated bytes; wmbus_line.stream is the capture and .channel the channel, captures ascending, channels
    ascending within a capture."""
    caps, hz = wide["caps"], CF.WIDE_HZ
    push_bytes = push or caps[0].size
    kw = dict(max_push_bytes=caps[0].size if push is None else 1 << 18, line_levels=1, rounds_on_host=rounds_on_host, **WIDE_KW)
    single = []
    for f in hz:
        with wm.Receiver(n_streams=2, input_shift_hz=f, **kw) as rx:
            text, levels, _ = run_with_levels(rx, caps, push_bytes, 2)
            chips = [rx.read_chips(0, 1, k) for k in range(2)] + [rx.read_chips(1, 0, k) for k in range(2)]
            single.append((text, levels, chips))
    with wm.Receiver(n_streams=2, input_channel_hz=hz, **kw) as rx:
        text, levels, keys = run_with_levels(rx, caps, push_bytes, 6)
        for k in range(2):
            for c in range(3):
                v = k * 3 + c
                assert text[v] == single[c][0][k], (k, c)
                assert text[v] == wide["text"][k][c], (k, c)
                assert levels[v] == single[c][1][k], (k, c)
                for j, (chain, algo) in enumerate(((0, 1), (1, 0))):
                    w, pos = rx.read_chips(chain, algo, v)
                    sw, spos = single[c][2][2 * j + k]
                    assert np.array_equal(w, sw) and np.array_equal(pos, spos), (k, c, chain, algo)
        assert rx.resampler_launches() == -(-caps[0].size // push_bytes)
    assert len(text[0].splitlines()) >= 6 and len(text[1].splitlines()) >= 6 and len(text[2].splitlines()) >= 6
    # the second capture is the first with channels 0 and 1 swapped: another capture's telegrams on the same channel (the texts above are
    # the oracle's per capture and channel, so a line filed under the wrong capture or channel has already failed)
    assert text[3] != text[0] and text[4] != text[1]
    if push is None:                                         # one push: the order of wmbus_lines is (capture, channel), both ascending
        assert keys == sorted(keys) and set(keys) == {(k, c) for k in range(2) for c in range(3)}


# ---- 3. the bundled wideband capture ------------------------------------------------------------------------------------------------

def test_bundled_868_625_capture_at_its_two_centres_without_s(wm, oracle, samples):
    """issue48: 2.4 MS/s at 868.625 MHz, the capture the reference wants -s for.  Channels +325 kHz (T1/C1 at 868.95) and -325 kHz (S1 at
    868.30), decimation 3, no -s: each channel's text is the oracle's on the restated bytes and the single-shift context's.  Parity only:
    nobody has checked what this short capture yields per channel."""
    cu8 = samples["issue48"]
    cu8 = cu8[:cu8.size // BLK * BLK]
    hz = [325000, -325000]
    kw = dict(n_streams=1, max_push_bytes=cu8.size, decimation=3)
    with wm.Receiver(input_channel_hz=hz, **kw) as rx:
        got = rx.run(cu8)
        assert len(got) == 2
        bytes_ = [rx.read_resampled(v) for v in range(2)]
    for c, f in enumerate(hz):
        want = SR.pipeline_bytes(cu8, FR.CU8, 2400000, f)
        assert np.array_equal(bytes_[c], want)
        assert got[c] == oracle.run(np.ascontiguousarray(want), oracle.make_opts(decimation=3))["text"], f
        with wm.Receiver(input_shift_hz=f, **kw) as rx:
            assert rx.run(cu8)[0] == got[c], f
    print("issue48 lines per channel:", [len(t.splitlines()) for t in got])


# ---- 4. the blocker and the AGC ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["dc", "agc", "both"])
def test_blocker_and_agc_are_taken_once_per_capture(wm, wide, mode):
    """On the two cs16 captures: every channel's bytes equal the restatement's, and read_input_dc(k) / read_input_gain(k) take the CAPTURE
    and equal the restatement's and a single-shift context's."""
    caps, (L, M, taps) = wide["caps"], wide["taps"]
    R, agc = (6 if mode != "agc" else 0), (1 if mode != "dc" else 0)
    kw = dict(n_streams=2, max_push_bytes=caps[0].size, input_rate_hz=CF.WIDE_FS, input_format=FR.CS16, input_dc=R, input_agc=agc,
              input_gain_q8=0 if agc else CF.WIDE_GAIN)
    with wm.Receiver(input_shift_hz=CF.WIDE_HZ[0], **kw) as rx:
        rx.push(caps)
        single_dc = [rx.read_input_dc(k) for k in range(2)] if R else None
        single_g = [rx.read_input_gain(k) for k in range(2)] if agc else None
        single_clips = rx.timing()["input_clipped"]
    with wm.Receiver(input_channel_hz=CF.WIDE_HZ, **kw) as rx:
        rx.push(caps)
        clips = 0
        for k in range(2):
            for c, f in enumerate(CF.WIDE_HZ):
                want, n_clip, dc, g = CF.restated(caps[k], FR.CS16, CF.WIDE_FS, f, CF.WIDE_GAIN, L, M, taps, R, agc)
                assert np.array_equal(rx.read_resampled(k * 3 + c), CF.whole_blocks(want)), (k, c)
                clips += n_clip
            if R:
                got = rx.read_input_dc(k)
                assert np.array_equal(got, dc) and np.array_equal(got, single_dc[k]), k
            if agc:
                got = rx.read_input_gain(k)
                assert np.array_equal(got, g) and np.array_equal(got, single_g[k]), k
        assert rx.timing()["input_clipped"] == clips
        for read in ([rx.read_input_dc] if R else []) + ([rx.read_input_gain] if agc else []):
            with pytest.raises(wm.WmbusError):
                read(2)                                      # by capture: there are two, not six
    assert single_clips <= clips


# ---- 5. a batch -------------------------------------------------------------------------------------------------------------------

FIVE_HZ, FIVE_PUSH = [200000, -150000], 1 << 18
_FIVE = {}


def five_captures(wm):
    """The five captures of the batch tests and, per (capture, channel), the text of a single context with that channel's fixed shift in
    pushes of 2^18 bytes: computed once, shared, left unchanged."""
    if not _FIVE:
        cu8s = [wm.synth_capture(seed=9300 + k, n_samples=1 << 18, kinds=15, frames_per_s=80.0)[0] for k in range(5)]
        caps = [SR.round_trip_cu8(c, OUT_HZ, FIVE_HZ[k % 2]) for k, c in enumerate(cu8s)]
        want = {}
        for c, f in enumerate(FIVE_HZ):
            with wm.Receiver(n_streams=5, input_shift_hz=f, keep_taps=False, max_push_bytes=FIVE_PUSH, input_gain_q8=SR.CU8_ROUND_TRIP_GAIN) as rx:
                for k, t in enumerate(rx.run(caps, push_bytes=FIVE_PUSH)):
                    want[(k, c)] = t
        assert all(len(want[(k, k % 2)].splitlines()) >= 3 for k in range(5))
        for c in caps:
            c.setflags(write=False)
        _FIVE.update(caps=caps, want=want)
    return _FIVE["caps"], _FIVE["want"]


def test_batch_of_five_captures_and_two_channels_in_one_lane(wm):
    """The batch below with its two contexts (3 + 2 captures, two channels each) in ONE lane, two pushes: the channel form of the input
    kernel recorded and issued behind the mate's operations, two mates of different widths in every paired launch."""
    caps, want = five_captures(wm)
    got = one_lane(wm, caps, 5, push=FIVE_PUSH, n_push=caps[0].size // FIVE_PUSH, input_windows=2, input_channel_hz=FIVE_HZ, input_gain_q8=SR.CU8_ROUND_TRIP_GAIN)
    assert got.plan == [(0, 3), (3, 2)] and caps[0].size // FIVE_PUSH == 2 and got.run_stats["samples"] == 5 * caps[0].size // 2
    text = {(k, c): "".join(ln["text"] for push in got.lines[k] for ln in push if ln["channel"] == c) for k in range(5) for c in range(2)}
    assert text == want


def test_batch_of_five_captures_and_two_channels(wm, oracle):
    """Five native-rate cu8 captures through a fill source, two contexts: captures 0, 2, 4 were mixed up by 200 kHz, 1 and 3 down by
    150 kHz.  The sink sees stream 0 ... 4 (batch-wide) and channel 0 ... 1 with the single-context text of every pair."""
    hz, push, kw = FIVE_HZ, FIVE_PUSH, dict(max_push_bytes=FIVE_PUSH, input_gain_q8=SR.CU8_ROUND_TRIP_GAIN)
    caps, want = five_captures(wm)
    got = {(k, c): "" for k in range(5) for c in range(2)}
    with wm.Batch(n_streams=5, contexts=2, input_windows=2, input_channel_hz=hz, **kw) as b:
        assert [n for _, _, n in b.contexts] == [3, 2]       # the plan splits captures
        pos = {}

        def fill(first, n, slab):
            off = pos.get(first, 0)
            k = min(push, caps[0].size - off)
            for s in range(n):
                slab[s, :k] = caps[first + s][off:off + k]
            pos[first] = off + k
            return k

        def on_push(first, n, lines, tm):
            seen = [(ln["stream"], ln["channel"]) for ln in lines]
            assert seen == sorted(seen)
            for ln in lines:
                assert first <= ln["stream"] < first + n and ln["channel"] < 2
                got[(ln["stream"], ln["channel"])] += ln["text"]
        st = b.run_from(fill, on_push)
        assert st["samples"] == 5 * caps[0].size // 2        # captures, not pipeline streams
    assert got == want


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------------

def split_channels(out, hz):
    """The CLI's lines by their last field, that field stripped; every line must carry one of the channels."""
    per = {f: "" for f in hz}
    for line in out.splitlines():
        body, _, last = line.rpartition(";")
        per[int(last)] += body + "\n"
    return per


def test_cli_takes_a_list_of_offsets(wm, wide, tmp_path):
    assert int(np.rint(256.0 * 10.0 ** (float(GAIN_DB) / 20.0))) == CF.WIDE_GAIN          # wm_main.c, -g
    caps, hz = wide["caps"], CF.WIDE_HZ
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    base = [wm.CLI_PATH, "-R", "4M", "-I", "cs16", "-g", GAIN_DB, "-v"]
    # the whole capture in one push: channels ascending, within a channel the oracle's order
    p = subprocess.run(base + ["-O", "700k,-600k,0", "-B", str(caps[0].size), "-L", "0"], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    want = "".join(ln + ";" + str(f) + "\n" for c, f in enumerate(hz) for ln in wide["text"][0][c].splitlines())
    assert p.stdout.decode() == want
    assert [ln.rsplit(";", 1)[1] for ln in want.splitlines()] == ["700000"] * 8 + ["-600000"] * 10 + ["0"] * 6
    # the default pushes: the same lines per channel
    p = subprocess.run(base + ["-O", "0.7M,-600000,0"], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert split_channels(p.stdout.decode(), hz) == {f: wide["text"][0][c] for c, f in enumerate(hz)}
    # -l: the channel stands behind the two level fields
    p = subprocess.run(base + ["-O", "700k,-600k,0", "-l"], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    per = split_channels(p.stdout.decode(), hz)
    for c, f in enumerate(hz):
        rows = [ln.split(";") for ln in per[f].splitlines()]
        assert all(r[-2] == "" or int(r[-2]) is not None for r in rows)      # offset_hz (empty where the preamble lies before the stream)
        assert all(r[-1] == "" or int(r[-1]) >= 0 for r in rows)             # dev_hz
        assert "".join(";".join(r[:-2]) + "\n" for r in rows) == wide["text"][0][c]
    p = subprocess.run(base + ["-O", "700k", "-l"], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.decode() == per[hz[0]]     # the single shift's lines and levels, field for field
    # batch mode, two files
    caps[0].tofile(tmp_path / "a.cs16"); caps[1].tofile(tmp_path / "b.cs16")
    p = subprocess.run(base + ["-O", "700k,-600k,0", "-S", "-G", "0", "a.cs16", "b.cs16"], cwd=tmp_path, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    got = {"a.cs16": "", "b.cs16": ""}
    for line in p.stdout.decode().splitlines(True):
        name, rest = line.split(": ", 1)
        got[name] += rest
    for k, name in enumerate(("a.cs16", "b.cs16")):
        assert split_channels(got[name], hz) == {f: wide["text"][k][c] for c, f in enumerate(hz)}, name
    # one entry is the shift it always was: no field appended
    p = subprocess.run(base + ["-O", "700k"], input=caps[0].tobytes(), capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == wide["text"][0][0]
    # nine entries, an empty entry and an entry beyond half the rate
    for bad in ("0,1,2,3,4,5,6,7,8", "700k,,0", "700k,", ",700k", "700k,foo"):
        p = subprocess.run(base + ["-O", bad], input=b"", capture_output=True, env=env)
        assert p.returncode == 1 and "Usage" in p.stdout.decode(), bad
    p = subprocess.run(base + ["-O", "700k,-2.1M"], input=b"", capture_output=True, env=env)
    assert p.returncode == 1 and b"2000000" in p.stderr


# ---- 7. no channels: the context it always was ---------------------------------------------------------------------------------------

def test_no_channels_is_the_plain_path(wm, oracle, samples):
    cu8 = samples["samples2"]
    want = BUNDLED["rtlsdr_868.950M_1M6_samples2.cu8|-v"]
    assert len(want.splitlines()) >= 4
    for kw in (dict(), dict(input_channel_hz=None), dict(input_channel_hz=[])):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 20, **kw) as rx:
            assert rx.cfg.input_channels == 0
            assert rx.run(cu8)[0] == want
            assert rx.resampler_launches() == 0
            assert all(ln["channel"] == 0 and ln["stream"] == 0 for ln in rx.lines())
            tm = rx.timing()
            assert tm["input_clipped"] == 0 and tm["input_bytes_out"] == 0
            with pytest.raises(wm.WmbusError):
                rx.read_resampled(0)
    # one channel at 0 Hz on plain cu8 is a stage, and by the 0 Hz identity it hands on the capture itself
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 20, input_channel_hz=[0]) as rx:
        assert rx.run(cu8)[0] == want
        assert rx.resampler_launches() == cu8.size // (1 << 20)
        assert np.array_equal(rx.read_resampled(0), cu8[-(1 << 20):]) and rx.timing()["input_clipped"] == 0


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused(wm):
    bad = [(dict(input_channel_hz=[1000 * k for k in range(9)]), "input_channels"),
           (dict(input_channel_hz=[325000, -325000], input_shift_hz=5), "input_shift_hz"),
           (dict(input_channel_hz=[0, 800001]), r"input_channel_hz\[1\]"),
           (dict(input_channel_hz=[-1024001], input_rate_hz=2048000), r"input_channel_hz\[0\]")]
    for open_ in (lambda **kw: wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw), lambda **kw: wm.Batch(n_streams=8, max_push_bytes=1 << 16, **kw)):
        for kw, field in bad:
            with pytest.raises(wm.WmbusError, match=field) as e:
                open_(**kw)
            assert "(-1)" in str(e.value), str(e.value)          # WMBUS_EINVAL; the handle was closed behind the message
    # the pipeline's width is n_streams x input_channels: refused before anything is allocated, naming both
    with pytest.raises(wm.WmbusError, match="n_streams x input_channels") as e:
        wm.Receiver(n_streams=1 << 27, max_push_bytes=1 << 16, input_channel_hz=[0] * 8)
    assert "(-1)" in str(e.value)
    for kw in (dict(input_channel_hz=[800000, -800000, 0, 0]), dict(input_channel_hz=[-1024000], input_rate_hz=2048000, input_format=wm.FMT_CF32),
               dict(input_channel_hz=list(range(8)))):
        with wm.Receiver(n_streams=1, max_push_bytes=1 << 16, **kw) as rx:
            assert rx.n_channels == len(kw["input_channel_hz"])
    with wm.Receiver(n_streams=2, max_push_bytes=1 << 16, input_channel_hz=[1, 2, 3]) as rx:      # by capture / by pipeline stream
        assert rx.device_input(1) and not rx.device_input(2)
        with pytest.raises(wm.WmbusError):
            rx.stage(2, np.zeros(4096, np.uint8))
