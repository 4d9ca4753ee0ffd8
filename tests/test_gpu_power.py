"""Channel power on the GPU (cfg.line_power): the band rows and the channel power of every pipeline row equal tests/power_ref.py, the
records do not depend on how the input is cut into pushes nor on any gain, and nothing else of a context moves."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import afc_age_ref as AG
import format_ref as FR
import power_ref as PW
import spectrum_ref as PR
from lanes import one_lane
from test_formats_emulated import FMT_IDS, FORMATS
from test_power_emulated import level_blocks

pytestmark = pytest.mark.gpu

FS = 1600000
CUTS = [1, 3, 16, 5, 64, 7]                         # 4096-byte units per push, repeated until the capture ends
# The generator's own figure for amplitude 60, sigma 3 through the window of nb of the 32 bands: A^2 / (2 sigma^2 nb / 32) = 1280 (31.1 dB).
# tests/power_ref.py on the generator's frames of seeds 1 ... 8 (67 telegrams, CPU): the worst deviation is 1.18 dB,
# on the 63 whose noise window is not wholly covered by another telegram (the other 4 read x 1: the rule's limit); the bound is twice that.  Seed 1's own worst is 0.56 dB on the frames, 0.65 dB on the lines of the GPU run.
SEED, AMPLITUDE, SIGMA = 1, 60.0, 3.0
WORST_DB = 1.18


def cut_sizes(total, cuts=CUTS):
    out, left, k = [], total // 4096 * 4096, 0
    while left:
        n = min(4096 * cuts[k % len(cuts)], left)
        out.append(n); left -= n; k += 1
    return out


def run_power(wm, caps, sizes, afc=False, **kw):
    """All pushes of `caps` through one context.  Returns a dict: lines = [(line, level, power)] in order, P[(chain, v)] = the row's
    timeline over the whole stream, rows[capture] = the waterfall of the whole stream, firsts = the first level block of every push,
    locks = read_input_afc of every push (afc), survey[capture] = read_spectrum at the end."""
    kw.setdefault("line_power", 1)
    kw.setdefault("keep_taps", False)
    out = dict(lines=[], P={}, rows={}, firsts=[], locks=[], survey={})
    with wm.Receiver(n_streams=len(caps), max_push_bytes=max(sizes), **kw) as rx:
        S = len(caps) * rx.n_channels
        off = 0
        for n in sizes:
            rx.push([c[off:off + n] for c in caps]); off += n
            lines, levels, powers = rx.lines(), rx.line_levels(), rx.line_power()
            assert len(lines) == len(levels) == len(powers)
            out["lines"] += list(zip(lines, levels, powers))
            first = None
            for ch in (0, 1):
                for v in range(S):
                    p, f = rx.read_channel_power(ch, v)
                    assert first in (None, f)
                    first = f
                    out["P"].setdefault((ch, v), []).append(p)
            for k in range(len(caps)):
                rows, f = rx.read_waterfall(k)
                assert f == first and rows.shape[0] == p.size
                out["rows"].setdefault(k, []).append(rows)
            out["firsts"].append(first)
            if afc:
                out["locks"].append(rx.read_input_afc(0))
        for k in range(len(caps)):
            out["survey"][k] = rx.read_spectrum(k)
    out["P"] = {k: np.concatenate(v) for k, v in out["P"].items()}
    out["rows"] = {k: np.concatenate(v) for k, v in out["rows"].items()}
    return out


def records_equal_the_rule(run, fin, d=2, L=1, M=1, S=1):
    for ln, lv, pw in run["lines"]:
        v = ln["stream"] * (S // max(1, len(run["rows"]))) + ln["channel"]
        ka, ke = PW.block_of(lv["sync_sample"], d, L, M), PW.block_of(ln["sample"], d, L, M)
        assert pw == PW.line_record(run["P"][(ln["chain"], v)], 0, ka, ke, fin), (ln, lv, pw)


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_waterfall(wm, fmt):
    """1.  Three captures of 2^15 samples (random, silent, tone) in two pushes: the rows equal tests/power_ref.py; P of the centred row
    equals it too; and against the survey that is already trusted: the rows summed over all pushes are wmbus_read_spectrum's sum grouped
    by 16 bins (no band clamps: test_power_emulated.py says why none can)."""
    n_blk = (1 << 15) // PR.N
    caps = [level_blocks(fmt, n_blk, kind) for kind in ("random", "silence", "tone")]
    got = run_power(wm, caps, [4096 * 3, caps[0].size - 4096 * 3], input_format=fmt)
    assert got["firsts"] == [0, 4096 * 3 // FR.BPS[fmt] // PR.N]
    for k, raw in enumerate(caps):
        want = PW.band_rows(raw, fmt)
        assert got["rows"][k].shape == want.shape and np.array_equal(got["rows"][k], want), k
        assert int(want.max()) < PW.U32
        total, peak, blocks = got["survey"][k]
        assert blocks == n_blk and np.array_equal(got["rows"][k].astype(np.uint64).sum(axis=0), total.reshape(32, 16).sum(axis=1))
        for ch in (0, 1):
            assert np.array_equal(got["P"][(ch, k)], PW.channel_power(want, FS, 0))


@pytest.fixture(scope="module")
def capture(wm):
    """The synthetic capture of tests 2, 4, 5 and 6, its reference rows and timeline, and one push of it: computed once, left unchanged."""
    cu8, frames = wm.synth_capture(seed=SEED, n_samples=1 << 19, kinds=wm.T1 | wm.C1A | wm.S1, frames_per_s=40.0, amplitude=AMPLITUDE, noise_sigma=SIGMA)
    rows = PW.band_rows(cu8, FR.CU8)
    return dict(cu8=cu8, frames=frames, rows=rows, P=PW.channel_power(rows, FS, 0), one=run_power(wm, [cu8], [cu8.size], line_levels=1))


def test_cut_independence(wm, capture):
    """2.  Pushed once, and in pushes of 4096 x {1, 3, 16, 5, 64, 7} bytes, the latter also with every burst through the host decoders and
    with every hand-off round on the host: the same timelines, the same records, and both equal to tests/power_ref.py."""
    cu8, one = capture["cu8"], capture["one"]
    sizes = cut_sizes(cu8.size)
    assert np.array_equal(one["rows"][0], capture["rows"])
    for ch in (0, 1):
        assert np.array_equal(one["P"][(ch, 0)], capture["P"])
    records_equal_the_rule(one, FS)
    assert len(one["lines"]) >= 12
    for kw in (dict(), dict(bursts_to_host=True), dict(rounds_on_host=True)):
        cut = run_power(wm, [cu8], sizes, line_levels=1, **kw)
        assert np.array_equal(cut["rows"][0], capture["rows"]) and all(np.array_equal(cut["P"][(ch, 0)], capture["P"]) for ch in (0, 1)), kw
        assert cut["firsts"] == [int(v) for v in np.cumsum([0] + [n // 1024 for n in sizes[:-1]])]
        assert cut["lines"] == one["lines"], kw
        # at least one telegram has its access code and its end in different pushes
        edges = np.cumsum([n // 2 // 2 for n in sizes])                  # decimated samples
        assert any(np.searchsorted(edges, lv["sync_sample"], "right") != np.searchsorted(edges, ln["sample"], "right") for ln, lv, _ in cut["lines"]), kw


def test_in_one_batch_lane(wm, capture):
    """The stage in a batch lane: the capture of test 2 and a second one (seed 2), each in both of two contexts that share ONE lane, four
    pushes of 2^18 bytes -- the band form of the survey, k0_channel_power and the copy of P to the host recorded and issued behind the
    mate's operations.  Every line's record equals tests/power_ref.py's rule on the restated timeline of its capture, the lines and records
    of the first capture are those of test 2's single context, and everything equals the lane-per-context run."""
    other = wm.synth_capture(seed=SEED + 1, n_samples=1 << 19, kinds=wm.T1 | wm.C1A | wm.S1, frames_per_s=40.0, amplitude=AMPLITUDE, noise_sigma=SIGMA)[0]
    caps = [capture["cu8"], other]
    P = [capture["P"], PW.channel_power(PW.band_rows(other, FR.CU8), FS, 0)]
    got = one_lane(wm, caps + caps, 4, push=1 << 18, n_push=caps[0].size >> 18, input_windows=2, line_power=1, line_levels=1)
    assert got.plan == [(0, 2), (2, 2)] and caps[0].size >> 18 == 4
    for s in range(4):
        recs = [r for push in got.lines[s] for r in push]
        want = [PW.line_record(P[s % 2], 0, PW.block_of(r["level"]["sync_sample"]), PW.block_of(r["sample"]), FS) for r in recs]
        assert len(recs) >= 5 and any(w["n_signal"] for w in want)           # lines, and records that are not empty, in every context
        assert [r["power"] for r in recs] == want, s
        if s % 2 == 0:
            assert [(r["text"], r["level"], r["power"]) for r in recs] == [(ln["text"], lv, pw) for ln, lv, pw in capture["one"]["lines"]]


def test_windows_shift_channels_and_simultaneous(wm):
    """3a.  P of every row equals tests/power_ref.py on the capture's rows for a fixed input_shift_hz, for two channels of a 4.0 MS/s cs16
    capture, and with -s, where the two chains' rows differ by the +-325 kHz."""
    rng = np.random.default_rng(33)
    # a tilted spectrum, so that a window one band off shows: noise plus three tones
    def tilted(fin, n):
        t = np.arange(n)
        x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        for f, a in ((-0.31 * fin, 0.3), (0.07 * fin, 0.2), (0.4 * fin, 0.25)):
            x = x + a * np.exp(2j * np.pi * f / fin * t)
        return np.stack([x.real, x.imag], axis=1).reshape(-1)
    n = 1 << 15
    cu8 = np.clip(np.rint(127.5 + 127.5 * tilted(FS, n)), 0, 255).astype(np.uint8)
    got = run_power(wm, [cu8], [4096 * 5, cu8.size - 4096 * 5], input_shift_hz=-123456)
    rows = PW.band_rows(cu8, FR.CU8)
    assert np.array_equal(got["rows"][0], rows)
    for ch in (0, 1):
        assert np.array_equal(got["P"][(ch, 0)], PW.channel_power(rows, FS, -123456))
    assert not np.array_equal(PW.channel_power(rows, FS, -123456), PW.channel_power(rows, FS, 0))

    fin, hz = 4000000, [1600000, -1240000]
    cs16 = FR.raw_bytes(np.clip(np.rint(32767 * tilted(fin, n)), -32768, 32767), FR.CS16)
    got = run_power(wm, [cs16, cs16[::-1].copy()], [cs16.size], input_rate_hz=fin, input_format=FR.CS16, input_channel_hz=hz)
    for k, raw in enumerate((cs16, cs16[::-1].copy())):
        rows = PW.band_rows(raw, FR.CS16)
        assert np.array_equal(got["rows"][k], rows)
        for c, f in enumerate(hz):
            for ch in (0, 1):
                assert np.array_equal(got["P"][(ch, 2 * k + c)], PW.channel_power(rows, fin, f)), (k, c, ch)
    assert PW.centre(fin, hz[0])[2] != PW.centre(fin, hz[1])[2]

    fin = 2400000
    cu8 = np.clip(np.rint(127.5 + 127.5 * tilted(fin, n)), 0, 255).astype(np.uint8)
    got = run_power(wm, [cu8], [cu8.size], decimation=3, simultaneous=True)
    rows = PW.band_rows(cu8, FR.CU8)
    want = [PW.channel_power(rows, fin, PW.chain_hz(ch, True)) for ch in (0, 1)]
    assert np.array_equal(got["P"][(0, 0)], want[0]) and np.array_equal(got["P"][(1, 0)], want[1]) and not np.array_equal(want[0], want[1])
    assert PW.centre(fin, 325000)[2] > PW.centre(fin, -325000)[2]


def test_windows_follow_the_afc_lock(wm):
    """3b.  input_afc on the two-tone capture of the ageing tests, whose lock changes between pushes: P of each push equals
    tests/power_ref.py evaluated with the shift_hz wmbus_read_input_afc reports for that push."""
    raw, cuts = AG.two_tones()
    got = run_power(wm, [raw], cuts, afc=True, input_afc=1, input_spectrum_age=6)
    rows = PW.band_rows(raw, FR.CU8)
    assert np.array_equal(got["rows"][0], rows)
    shifts = [lk["shift_hz"] for lk in got["locks"]]
    assert len(set(shifts)) >= 2 and got["locks"][-1]["changes"] >= 2, shifts
    off = 0
    for n, f in zip(cuts, shifts):
        nb = n // 2 // PR.N
        for ch in (0, 1):
            assert np.array_equal(got["P"][(ch, 0)][off:off + nb], PW.channel_power(rows[off:off + nb], FS, f)), (off, f)
        off += nb
    assert PW.centre(FS, shifts[0])[2] != PW.centre(FS, shifts[-1])[2] or shifts[0] == shifts[-1]


def test_meaning(capture):
    """4.  Every CRC-clean line whose telegram starts more than G + Nn level blocks into the stream has a full noise window and at least
    one signal block, and its ratio lies within twice the restatement's own worst deviation (1.18 dB on seeds 1 ... 8, DESIGN.md
    section 6) of the generator's figure amplitude^2 / (2 sigma^2 nb / 32)."""
    G, Nn = PW.guard(FS)
    figure = AMPLITUDE ** 2 / (2 * SIGMA ** 2 * PW.window(FS)[1] / 32)
    seen = 0
    for ln, lv, pw in capture["one"]["lines"]:
        if not ln["crc_ok"] or pw["first_block"] <= G + Nn:
            continue
        db = 10 * math.log10(pw["ratio_q8"] / 256 / figure) if pw["ratio_q8"] else -math.inf
        print(f"chain {ln['chain']} algo {ln['algo']} block {pw['first_block']}: x{pw['ratio_q8'] / 256:.1f}, {db:+.2f} dB of the figure")
        assert pw["n_noise"] == Nn and pw["n_signal"] >= 1, pw
        assert abs(db) <= 2 * WORST_DB, (ln, pw, db)
        seen += 1
    assert seen >= 8


def test_in_front_of_every_gain(wm, capture):
    """5.  The same capture with input_agc = 1, with input_gain_q8 = 64 and with neither: the power records of the lines common to all
    three are identical while their printed rssi differs."""
    cu8 = capture["cu8"]
    key = lambda ln: (ln["sample"], ln["chain"], ln["algo"])
    runs = [{key(ln): (ln, pw) for ln, _, pw in r["lines"]} for r in
            (capture["one"], run_power(wm, [cu8], [cu8.size], input_agc=1), run_power(wm, [cu8], [cu8.size], input_gain_q8=64))]
    common = set(runs[0]) & set(runs[1]) & set(runs[2])
    assert len(common) >= 6
    rssi = lambda ln: ln["text"].split(";")[5]                    # algorithm;mode;crc;3of6;timestamp;rssi;...
    for k in common:
        assert runs[0][k][1] == runs[1][k][1] == runs[2][k][1], k
    assert all(len({rssi(r[k][0]) for r in runs}) >= 2 for k in common)


def test_nothing_else_moves(wm, capture):
    """6.  Lines and level records with line_power = 1 equal those with 0; with 0 the three reads return WMBUS_EINVAL and wmbus_line_power
    returns 0 and a NULL array; anything above 1 is refused."""
    cu8, one = capture["cu8"], capture["one"]
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, keep_taps=False, line_levels=1) as rx:
        rx.push([cu8])
        assert rx.lines() == [ln for ln, _, _ in one["lines"]] and rx.line_levels() == [lv for _, lv, _ in one["lines"]]
        assert rx.line_power() == []
        p = ctypes.POINTER(wm.Power)()
        assert wm.lib().wmbus_line_power(rx._h, ctypes.byref(p)) == 0 and not p
        buf, first = np.zeros(64, np.uint32), ctypes.c_uint64()
        assert wm.lib().wmbus_read_waterfall(rx._h, 0, buf.ctypes.data, ctypes.byref(first), 2) == -1
        assert wm.lib().wmbus_read_channel_power(rx._h, 0, 0, buf.ctypes.data, ctypes.byref(first), 64) == -1
        with pytest.raises(wm.WmbusError):
            rx.read_spectrum(0)                                   # nothing switched the survey on either
    with pytest.raises(wm.WmbusError):
        wm.Receiver(n_streams=1, line_power=2)
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, keep_taps=False, line_power=1) as rx:      # line_power alone: the levels work too
        rx.push([cu8])
        assert rx.line_levels() == [lv for _, lv, _ in one["lines"]] and rx.line_power() == [pw for _, _, pw in one["lines"]]


def test_cli_switch(wm, capture, tmp_path):
    """7.  -n alone, with -l, with a channel list and in -S batch mode: the fields' count and order, and the library's values."""
    cu8, one = capture["cu8"], capture["one"]
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    power = lambda pw: f";{pw['signal'] if pw['n_signal'] else ''};{pw['noise'] if pw['n_noise'] else ''};" + (f"x{pw['ratio_q8'] / 256:.1f}" if pw["n_signal"] and pw["n_noise"] else "")
    level = lambda lv: f";{lv['offset_hz']};{lv['dev_hz']}" if lv["n"] else ";;"
    plain = "".join(ln["text"] for ln, _, _ in one["lines"])
    want_n = "".join(ln["text"][:-1] + power(pw) + "\n" for ln, _, pw in one["lines"])
    want_ln = "".join(ln["text"][:-1] + level(lv) + power(pw) + "\n" for ln, lv, pw in one["lines"])

    def cli(*args, **kw):
        p = subprocess.run([wm.CLI_PATH, "-v", *args], capture_output=True, env=env, timeout=120, **kw)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.decode()
    assert cli(input=cu8.tobytes()) == plain
    assert cli("-n", input=cu8.tobytes()) == want_n
    assert cli("-l", "-n", input=cu8.tobytes()) == want_ln
    assert all(ln.count(";") == plain.splitlines()[0].count(";") + 3 for ln in want_n.splitlines())
    # a channel list: the channel's field stays last
    got = cli("-n", "-l", "-O", "0,40k", input=cu8.tobytes()).splitlines()
    assert len(got) >= len(one["lines"]) and all(ln.rsplit(";", 1)[1] in ("0", "40000") for ln in got)
    assert [ln.rsplit(";", 1)[0] for ln in got if ln.endswith(";0")] == want_ln.splitlines()
    cu8.tofile(tmp_path / "a.cu8")
    assert cli("-n", "-S", "a.cu8", cwd=tmp_path) == "".join("a.cu8: " + x + "\n" for x in want_n.splitlines())
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, env=env, timeout=60)
    assert p.stdout.decode().count("\t-n append ;signal;noise;x<strength>") == 1
