"""The PRODUCT's own entry points on the GPU (the headline rate was reachable only through bench.py):
wmbus_batch_* through the ctypes mirror and through `rtl_wmbus_hip FILE...`, and the live-stream behaviour of the CLI
behind a pipe (latency bound, -f, timestamps).  Everything is held against the oracle / the reference's goldens."""
import json
import os
import re
import subprocess
import threading
import time

import numpy as np
import pytest

from cases import flags_to_kwargs, flags_to_oracle_opts
from conftest import GOLDEN, SAMPLES

pytestmark = pytest.mark.gpu
BUNDLED = json.load(open(os.path.join(GOLDEN, "bundled.json")))
S2_NAME = "rtlsdr_868.950M_1M6_samples2.cu8"


def _split_by_file(stdout, names):
    got = {n: "" for n in names}
    for line in stdout.decode().splitlines(True):
        name, rest = line.split(": ", 1)
        got[name] += rest
    return got


def test_cli_batch_of_320_files_runs_on_several_contexts_and_matches_the_oracle(wm, oracle, tmp_path):
    """320 files = five 64-capture groups -> five receiver contexts on five worker threads inside ONE wmbus_batch, files of
    three different lengths (ragged ends padded inside a group), three pushes each: every file's lines are what the capture
    gives alone through the oracle."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    n_files, push = 320, 1 << 19
    lens = [3 * push // 2, 3 * push // 2 - 4096 * 7, push // 2 + 4096 * 3 + 100]          # IQ samples x 2 bytes; the last one has a partial tail
    caps = [wm.synth_capture(seed=9000 + i, n_samples=lens[i % 3] // 2 + 50, kinds=15 if i % 4 else 7, frames_per_s=60.0)[0][:lens[i % 3]]
            for i in range(n_files)]
    names = [f"c{i:03d}.cu8" for i in range(n_files)]
    for nm, c in zip(names, caps):
        c.tofile(tmp_path / nm)
    want = dict(zip(names, oracle.run_many(caps, flags_to_oracle_opts(oracle, ["-v"]), threads=min(32, os.cpu_count() or 1))))
    p = subprocess.run([wm.CLI_PATH, "-v", "-S", "-B", str(push)] + names, cwd=tmp_path, capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert _split_by_file(p.stdout, names) == want
    assert sum(len(t) for t in want.values()) > 50000
    m = re.search(rb"320 files, (\d+) contexts, (\d+) samples", p.stderr)
    assert m and int(m.group(1)) == 5                          # the library split the batch, not the caller
    assert int(m.group(2)) == 320 * lens[0] // 2                 # every group advanced by its longest file


def test_cli_batch_set_up_stays_small_beside_the_decode(wm, tmp_path):
    """the reference starts decoding at its first read (rtl_wmbus.c:1298-1308).  320 files of 16 MiB (names linked
    onto eight captures): starting the HIP runtime and opening five contexts takes about as long as the decode, because the page-locked
    staging is pinned by the contexts' own threads while the first of them already decode (round 3 pinned everything first: 5-6 s
    of set-up before 1.6 s of decode for 1024 files)."""
    caps = [wm.synth_capture(seed=9500 + i, n_samples=1 << 23, kinds=7, frames_per_s=20.0)[0] for i in range(8)]
    for i, c in enumerate(caps):
        c.tofile(tmp_path / f"src{i}.cu8")
    names = []
    for i in range(320):
        os.symlink(tmp_path / f"src{i % 8}.cu8", tmp_path / f"f{i:03d}.cu8")
        names.append(f"f{i:03d}.cu8")
    runs = []
    for _ in range(3):                                         # the first run also loads the code objects and fills the page cache
        p = subprocess.run([wm.CLI_PATH, "-v", "-S"] + names, cwd=tmp_path, capture_output=True, env=dict(os.environ, WMBUS_FIXED_TS="1"), timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        t = re.search(rb"decode ([\d.]+) s = .*?with set-up .*? ([\d.]+) s =", p.stderr)
        assert t, p.stderr[-400:]
        runs.append((float(t.group(1)), float(t.group(2))))
    assert p.stdout.count(b"\n") > 10000
    # set-up (HIP start, five contexts opened side by side, lazily page-locked staging) is a fixed quarter of a second on a quiet box and the
    # decode of these 5.4 GB 0.22-0.25 s (round 6; tools/gpu_cli_setup.py prints both).  A clock inside a parity suite must not be tight:
    # the bound is the regression it guards against -- pinning everything before the first decode was 5-6 s -- not the quiet-box figure
    setup = min(w - d for d, w in runs[1:])
    assert setup <= 1.5, runs


def test_cli_batch_closes_its_batches_when_asked_to_exit_slowly(wm, oracle, tmp_path):
    """The batch CLI normally ends through _exit (the driver reclaims 60 GB faster than hipFree returns it); with
    WMBUS_SLOW_EXIT=1 every wmbus_batch is closed and the runtime's exit handlers run -- same output, exit code 0."""
    env = dict(os.environ, WMBUS_FIXED_TS="1", WMBUS_SLOW_EXIT="1")
    caps = [wm.synth_capture(seed=9900 + i, n_samples=1 << 18, kinds=15, frames_per_s=80.0)[0] for i in range(70)]
    names = [f"s{i:02d}.cu8" for i in range(70)]
    for nm, c in zip(names, caps):
        c.tofile(tmp_path / nm)
    want = dict(zip(names, oracle.run_many(caps, flags_to_oracle_opts(oracle, ["-v"]), threads=min(32, os.cpu_count() or 1))))
    p = subprocess.run([wm.CLI_PATH, "-v"] + names, cwd=tmp_path, capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert _split_by_file(p.stdout, names) == want


def test_batch_api_pipelines_pushes_and_keeps_every_stream_exact(wm, oracle):
    """wmbus_batch_run with a host source (two input windows, page-locked slabs filled by the callback) and with resident
    input: 192 captures in three contexts, five pushes each; the host decode of push k runs while push k + 1 is on the GPU,
    half-received telegrams cross the push boundaries (continuation bursts), and every stream's text over all pushes equals
    one oracle run over the whole capture."""
    S, push, n_push = 192, 1 << 18, 5
    caps = [wm.synth_capture(seed=7700 + i, n_samples=n_push * push // 2, kinds=15, frames_per_s=120.0)[0] for i in range(S)]
    want = oracle.run_many(caps, flags_to_oracle_opts(oracle, ["-v"]), threads=min(32, os.cpu_count() or 1))
    with wm.Batch(n_streams=S, max_push_bytes=push, input_windows=2) as b:
        assert len(b.contexts) == 3 and [c[2] for c in b.contexts] == [64, 64, 64]
        left = {first: 0 for _, first, _ in b.contexts}
        text = [[] for _ in range(S)]

        def fill(first, n, slab):
            k = left[first]
            if k == n_push:
                return 0
            left[first] = k + 1
            for j in range(n):
                slab[j, :push] = caps[first + j][k * push:(k + 1) * push]
            return push

        def on_push(first, n, lines, tm):
            assert tm["warnings"] == 0
            for ln in lines:
                assert first <= ln["stream"] < first + n
                text[ln["stream"]].append(ln["text"])
        st = b.run_from(fill, on_push)
        assert st["pushes"] == 3 * n_push and st["samples"] == S * n_push * push // 2
        assert ["".join(t) for t in text] == want
        assert st["lines"] == sum(len(t) for t in text)
    # resident input: the same bytes every pass, carried state of the earlier passes included
    with wm.Batch(n_streams=128, contexts=2, max_push_bytes=push) as b:
        for s in range(128):
            b.stage(s, caps[s][:push])
        seen = {}
        st = b.run_resident(push, 3, lambda first, n, lines, tm: seen.setdefault(first, []).append("".join(ln["text"] for ln in lines if ln["stream"] == first)))
        want3 = oracle.run_many([caps[f][:push] for f in sorted(seen)], flags_to_oracle_opts(oracle, ["-v"]), passes=3, threads=2)
        assert st["pushes"] == 6 and [seen[f][2] for f in sorted(seen)] == want3


def test_cli_live_stream_latency_is_bounded_by_L_not_by_the_push_size(wm, samples):
    """samples2 at its real rate (3.2 MB/s, 0.65 s of air time) into a 4 MiB push: nothing would come out before end of
    input without the latency bound.  With -L 40 every telegram is on stdout within 40 ms (+ the GPU's few milliseconds and
    scheduling slack) of the moment its completing sample was written into the pipe, and the text is the reference's."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    data = samples["samples2"].tobytes()
    with wm.Receiver(n_streams=1, max_push_bytes=len(data)) as rx:
        rx.push([samples["samples2"]])
        done_at_byte = [4 * ln["sample"] for ln in rx.lines()]           # decimated sample -> input byte (d = 2, 2 bytes per sample)
    p = subprocess.Popen([wm.CLI_PATH, "-v", "-B", str(4 << 20), "-L", "40"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    piece, sent = 16384, []

    def writer():
        for k in range(0, len(data), piece):
            os.write(p.stdin.fileno(), data[k:k + piece])
            sent.append(time.monotonic())                              # the piece is in the pipe (the first ones wait for the CLI's set-up)
            time.sleep(piece / 3.2e6)
        p.stdin.close()
    th = threading.Thread(target=writer)
    th.start()
    got, t_line = [], []
    for _ in done_at_byte:
        got.append(p.stdout.readline())
        t_line.append(time.monotonic())
    rest = p.stdout.read()
    th.join()
    assert p.wait() == 0, p.stderr.read()
    assert (b"".join(got) + rest).decode() == BUNDLED[f"{S2_NAME}|-v"] and rest == b""
    lat = [t - sent[min(b // piece, len(sent) - 1)] for t, b in zip(t_line, done_at_byte)]
    print("latency of the lines (s):", [round(x, 4) for x in lat])
    assert max(lat) < 0.040 + 0.150, lat                                  # 1 MiB pushes alone would make this up to 0.33 s, 4 MiB 0.65 s
    assert t_line[0] < sent[-1] - 0.1                                     # the first telegram is out long before the stream ends


def test_cli_f_decodes_what_it_has_read_before_giving_up(wm, samples):
    """-f (/root/reference/rtl_wmbus.c:61-79,1300-1308): the reference processes every block it has read before the alarm
    can fire; so do we -- the staged bytes are decoded, then the message, exit code 1."""
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    data = samples["samples2"].tobytes()
    p = subprocess.Popen([wm.CLI_PATH, "-v", "-f", "-L", "0"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    p.stdin.write(data[:len(data) // 4096 * 4096 - 4096 * 10]); p.stdin.flush()        # ... and then the flow stops, pipe still open
    t0 = time.monotonic()
    try:
        rc = p.wait(timeout=30)
    finally:
        p.stdin.close()
    out, err = p.stdout.read().decode(), p.stderr.read().decode()
    assert rc == 1 and 1.5 < time.monotonic() - t0 < 10
    assert "monitoring flow" in err and "exiting since incoming data stopped flowing" in err
    assert out == BUNDLED[f"{S2_NAME}|-v"]                        # all four telegrams end before the missing tail


def test_timestamps_follow_the_completing_sample(wm, samples):
    """Line time = hand-over time of the push - (push end - completing sample) / 800 kHz (the reference stamps at
    last-chip processing, t1_c1_packet_decoder.h:390,458): within one push the stamps of two lines differ by exactly their
    sample distance, and none lies after the hand-over."""
    import datetime
    with wm.Receiver(n_streams=1, max_push_bytes=samples["samples2"].size, fixed_timestamp=False) as rx:
        t_before = time.time()
        rx.push([samples["samples2"]])
        t_after = time.time()
        lines = rx.lines()
    assert len(lines) == 4
    ts = [datetime.datetime.strptime(ln["text"].split(";")[4], "%Y-%m-%d %H:%M:%S.%f").timestamp() for ln in lines]
    for a in range(4):
        for b in range(a + 1, 4):
            want = (lines[b]["sample"] - lines[a]["sample"]) / 800e3
            assert abs((ts[b] - ts[a]) - want) < 3e-6, (a, b, ts[b] - ts[a], want)
    m_end = samples["samples2"].size // 4
    assert t_before - 1e-3 <= ts[-1] + (m_end - 1 - lines[-1]["sample"]) / 800e3 <= t_after + 1e-3


@pytest.mark.parametrize("name,flags", [(S2_NAME, ["-v"]), ("rtlsdr_868.625M_2M4_issue48.cu8", ["-d", "3", "-s", "-o", "-v"])])
def test_tolerance_mode_keeps_the_bundled_datagrams_and_states_its_tolerance(wm, oracle, name, flags):
    """wmbus_cfg.tolerance_mode / CLI -F (never the default; BASELINE north_star allows "soft symbols within a stated float
    tolerance" as long as datagram bytes stay identical): polynomial arctangent + FMA low-passes.  On the reference's own
    captures the text is identical and every soft symbol lies within 2e-6 of the oracle's; RSSI bytes stay bit-identical."""
    from cases import flags_to_kwargs
    cu8 = np.fromfile(os.path.join(SAMPLES, name), np.uint8)
    ref = oracle.run(cu8, flags_to_oracle_opts(oracle, flags), taps=True)
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size // 4096 * 4096, tolerance_mode=1, **flags_to_kwargs(flags)) as rx:
        text = rx.run(cu8)[0]
        m = ref["m"]
        worst, differ = 0.0, 0
        for ch in (0, 1):
            d = rx.read_tap("dphi", ch, 0, m).astype(np.float64) - ref["dphi_fir"][ch].astype(np.float64)
            worst = max(worst, float(np.abs(d).max()))
            differ += int(np.count_nonzero(d))
            assert np.array_equal(rx.read_tap("rssi", ch, 0, m), ref["rssi"][ch].astype(np.uint32).astype(np.uint8))
    assert text == ref["text"] == BUNDLED[f"{name}|{' '.join(flags)}"]
    assert 0 < worst < 2e-6 and differ > m // 2                # really the other arithmetic, and within the stated tolerance
    env = dict(os.environ, WMBUS_FIXED_TS="1")
    p = subprocess.run([wm.CLI_PATH, "-F"] + flags, input=cu8.tobytes(), capture_output=True, env=env)
    assert p.returncode == 0 and p.stdout.decode() == ref["text"]


def test_rccl_group_works_next_to_the_hip_library(wm):
    """The process group bench.py uses for N > 1 (shard.init, backend nccl = RCCL) with ONE rank on this box, next to
    contexts of libwmbus_hip.so in the same process: barrier, max / sum reductions and the object gather all run, and a
    receiver opened afterwards still works (torch and the library share the HIP runtime).  The 8-rank run is the
    driver's; the transport's first contact with this process layout should not be there."""
    import importlib
    import subprocess
    import sys
    from conftest import ROOT
    code = (
        "import os, sys, importlib\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29547')\n"
        "shard = importlib.import_module('rtl-wmbus_amd.shard')\n"
        "g = shard.init(1, 0, backend='nccl', force=True)\n"
        "assert g.backend == 'nccl', g.backend\n"
        "shard.barrier(g)\n"
        "assert shard.max_over_ranks(g, 2.5) == 2.5 and shard.sum_over_ranks(g, 7) == 7 and shard.gather(g, [1, 2]) == [[1, 2]]\n"
        "wm = importlib.import_module('rtl-wmbus_amd')\n"
        "cu8 = wm.synth_capture(seed=5, n_samples=1 << 17, kinds=7, frames_per_s=100.0)[0]\n"
        "with wm.Receiver(n_streams=1, max_push_bytes=cu8.size) as rx:\n"
        "    n = len(rx.run(cu8)[0].splitlines())\n"
        "shard.barrier(g); shard.destroy(g)\n"
        "print('OK', n)\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    ok = [ln for ln in p.stdout.splitlines() if ln.startswith("OK ")]
    assert p.returncode == 0 and ok, p.stderr[-2000:]
    assert int(ok[0].split()[1]) > 0


def test_tolerance_mode_soft_symbols_do_not_depend_on_the_push_size(wm):
    """a repair launch of the RSSI filter (exact-zero input behind a signal, see
    test_signal_followed_by_exact_silence_repairs_the_rssi_filter) used to re-compute the repaired tiles' soft symbols with the
    EXACT kernel inside a tolerance-mode push -- which tiles are repaired depends on how the input is cut, so the soft
    symbols did too.  Repairs now leave the soft symbols alone: one push or eleven, every symbol is bit-identical."""
    sig, _ = wm.synth_capture(seed=77, n_samples=1 << 17, kinds=15, frames_per_s=120.0, amplitude=50.0)
    cu8 = np.concatenate([sig[: 37 * 4096], np.full(21 * 4096 + 2 * 977 * 2, 128, np.uint8), sig[37 * 4096: 90 * 4096], np.full(64 * 4096, 127, np.uint8),
                          sig[90 * 4096:]])
    cu8 = cu8[: cu8.size // 4096 * 4096]
    m = cu8.size // 4
    taps = []
    for push in (cu8.size, 24 * 4096):
        with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, tolerance_mode=1) as rx:
            got, retries, at = [[], []], 0, 0
            for off in range(0, cu8.size, push):
                n = min(push, cu8.size - off)
                rx.push([cu8[off:off + n]])
                retries += rx.timing()["ema_retries"]
                for ch in (0, 1):
                    got[ch].append(rx.read_tap("dphi", ch, 0, (off + n) // 4 - at))
                at = (off + n) // 4
            assert retries > 0                                   # the repair path ran
            taps.append([np.concatenate(g)[:m] for g in got])
    for ch in (0, 1):
        assert np.array_equal(taps[0][ch].view(np.uint32), taps[1][ch].view(np.uint32)), ch


def test_tolerance_mode_over_the_synthetic_goldens(wm):
    """Tolerance mode on every synthetic golden of the reference binary (tests/golden/synthetic.json; the switch
    combinations that do not run the default switches' kernel simply stay exact): the weak-signal and the all-modes cases
    are where a decision could hang on the last bits of a soft symbol.  The claim in DESIGN_HISTORY.md section 12 is "no line
    differs on these either"; a difference here is a finding about the mode, to be written down, not hidden."""
    from cases import SYNTH_CASES, flags_to_kwargs, synth_case_capture
    synth = json.load(open(os.path.join(GOLDEN, "synthetic.json")))
    differing = {}
    for case in SYNTH_CASES:
        cu8 = synth_case_capture(wm, case)[0]
        with wm.Receiver(n_streams=1, max_push_bytes=cu8.size // 4096 * 4096, tolerance_mode=1, keep_taps=False, **flags_to_kwargs(case["flags"])) as rx:
            text = rx.run(cu8)[0]
        if text != synth[case["id"]]:
            a, b = set(text.splitlines()), set(synth[case["id"]].splitlines())
            differing[case["id"]] = len(a ^ b)
    assert differing == {}, differing


def test_batch_api_argument_errors_and_odd_splits(wm, oracle):
    """Error behaviour of wmbus_batch_* (messages through wmbus_batch_last_error, nothing left half-open) and batches that do
    not split into whole 64-capture groups."""
    with pytest.raises(wm.WmbusError, match="n_streams"):
        wm.Batch(n_streams=0)
    with wm.Batch(n_streams=130, max_push_bytes=1 << 18) as b:           # a whole group of 64 + one context with the remainder (lane-private loads)
        assert [c[2] for c in b.contexts] == [64, 66]
        with pytest.raises(wm.WmbusError, match="input_windows"):
            b.run_from(lambda first, n, slab: 0)                           # a host source needs the second input window
        with pytest.raises(wm.WmbusError, match="resident_bytes"):
            b.run_resident(4096 * 3 + 1, 1)
        caps = [wm.synth_capture(seed=8800 + i, n_samples=1 << 17, kinds=15, frames_per_s=150.0)[0] for i in range(130)]
        for s, c in enumerate(caps):
            b.stage(s, c)
        text = [""] * 130
        def on_push(first, n, lines, tm):
            for ln in lines:
                text[ln["stream"]] += ln["text"]
        st = b.run_resident(1 << 18, 1, on_push)
        assert st["pushes"] == 2 and st["samples"] == 130 << 17
        assert text == oracle.run_many(caps, flags_to_oracle_opts(oracle, ["-v"]), threads=16)
    with wm.Batch(n_streams=64, max_push_bytes=1 << 16, input_windows=2) as b:
        with pytest.raises(wm.WmbusError, match="multiple of 4096"):
            b.run_from(lambda first, n, slab: 4097)                        # a source that returns a ragged byte count
        st = b.run_from(lambda first, n, slab: 0)                          # an empty source is not an error
        assert st["pushes"] == 0 and st["samples"] == 0


@pytest.mark.parametrize("caps", ["65536:300:65536:1048576", "65536:1048576:6:1048576", "65536:1048576:65536:200", "3:1048576:65536:1048576"],
                         ids=["words", "pkts", "bytes", "hdr"])
def test_exhausted_burst_storage_is_a_warning_and_never_hands_out_garbage(wm, oracle, caps):
    """with burst storage exhausted the K3 counters used to run ahead of what had been written, and the
    host walked unwritten slots of pinned memory.  Storage is now taken BEFORE a slot, a dropped continuation aborts its
    decoder, and the push succeeds with WMBUS_WARN_BURSTS_DROPPED: every line that still comes out is one of the oracle's
    (same text), none is invented, the stream goes on, and with the pressure gone (second receiver, default storage) the
    same bytes decode completely."""
    if os.environ.get("WMBUS_TEST_BURSTS_TO_HOST") == "1" and caps.split(":")[1] == "1048576":
        pytest.skip("every burst travels as chips in this campaign: packet / byte storage cannot run out")
    cu8 = wm.synth_capture(seed=4242, n_samples=1 << 20, kinds=15, frames_per_s=150.0)[0]
    want = oracle.run(cu8, flags_to_oracle_opts(oracle, ["-v"]))["text"].splitlines()
    code = (
        "import sys, importlib, json, numpy as np\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})\n"
        "wm = importlib.import_module('rtl-wmbus_amd')\n"
        "cu8 = wm.synth_capture(seed=4242, n_samples=1 << 20, kinds=15, frames_per_s=150.0)[0]\n"
        "out, warn = [], 0\n"
        "with wm.Receiver(n_streams=1, max_push_bytes=1 << 18, burst_caps=CAPS) as rx:\n"
        "    for off in range(0, cu8.size, 1 << 18):\n"
        "        out.append(rx.push([cu8[off:off + (1 << 18)]]))\n"
        "        warn |= rx.timing()['warnings']\n"
        "print('RESULT ' + json.dumps({'text': ''.join(out), 'warn': warn}))\n")
    import sys
    p = subprocess.run([sys.executable, "-c", code.replace("CAPS", repr([int(v) for v in caps.split(":")]))], capture_output=True, text=True, timeout=300)   # cfg.burst_caps
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    got = r["text"].splitlines()
    assert r["warn"] & 2                                      # WMBUS_WARN_BURSTS_DROPPED
    assert 0 < len(got) < len(want)
    it = iter(want)
    assert all(any(g == w for w in it) for g in got), "a line that the reference does not print, or out of order"
    p = subprocess.run([sys.executable, "-c", code.replace("CAPS", "None")], capture_output=True, text=True, timeout=300)
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert r["warn"] == 0 and r["text"].splitlines() == want


# ---- the product configuration (no debug views: RSSI on demand, the 2000-sample first pass) at BASELINE shape ----

def _batch_texts(b):
    per = {}
    for rx, first, _cnt in b.contexts:
        for ln in rx.lines():
            per.setdefault(first + ln["stream"], []).append(ln["text"])
    return per


def test_full_size_batch_in_the_product_configuration_matches_the_oracle(wm, oracle):
    """BASELINE configs[3] at an eighth of its width, the way bench.py, the CLI and wmbus_batch run it: 128 captures x 2^22 IQ
    samples in ONE context of a wm.Batch (keep_taps = 0: the first pass without the RSSI on 2000-sample tiles, k3_spans, the RSSI
    of the listed tiles).  Every capture's first push against the oracle; the third push of sixteen of them against an oracle
    fed the capture three times (the RSSI filter's state travels through `ema_out`, the framers' through their carries)."""
    n_streams, n = 128, 1 << 22
    caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, kinds=7, frames_per_s=20.0)[0] for s in range(n_streams)]
    want = oracle.run_many(caps, oracle.make_opts())
    tims = []
    with wm.Batch(n_streams=n_streams, contexts=1, max_push_bytes=2 * n) as b:
        assert len(b.contexts) == 1
        for s in range(n_streams):
            b.stage(s, caps[s])
        b.run_resident(2 * n, 1, on_push=lambda f, c, recs, tm: tims.append(tm), want_lines=False)
        got = _batch_texts(b)
        assert ["".join(got.get(s, [])) for s in range(n_streams)] == want
        b.run_resident(2 * n, 2, on_push=lambda f, c, recs, tm: tims.append(tm), want_lines=False)
        got3 = _batch_texts(b)
    picks = list(range(0, n_streams, 8))
    want3 = oracle.run_many([caps[s] for s in picks], oracle.make_opts(), passes=3)
    assert ["".join(got3.get(s, [])) for s in picks] == want3
    assert all(t["rssi_mode"] == wm.RSSI_ON_DEMAND and t["warnings"] == 0 for t in tims)      # a tenth of the tiles listed: never paused
    assert all(0 < t["rssi_tiles"] < 0.2 * n_streams * ((n // 2 + 975) // 976) for t in tims)
    if os.environ.get("WMBUS_TEST_ROUNDS_ON_HOST", "0") != "1":
        assert all(t["slow_path"] == 0 for t in tims)


@pytest.mark.parametrize("flags", [["-o", "-v"], ["-a", "-v"]], ids=["o-v", "a-v"])
def test_full_size_batch_with_the_dc_remover_and_the_fast_arctangent(wm, oracle, flags):
    """BASELINE shape (128 captures x 2^22 IQ samples, one context of a wm.Batch, no debug views) with -o -v -- the clock kernels'
    DC-remover instantiations, whose slicer words the run-length framer reads -- and with -a -v -- the reference's
    atan2_approximation kernels (rtl_wmbus.c:497-515,536-551; VERDICT r5 #5: these switches were covered at 128 x 2^18 and below).
    Every capture's first push and the second push of sixteen of them against the oracle."""
    n_streams, n = 128, 1 << 22
    caps = [wm.synth_capture(seed=0xBEEF00 + s, n_samples=n, kinds=7, frames_per_s=20.0)[0] for s in range(n_streams)]
    oo = flags_to_oracle_opts(oracle, flags)
    want = oracle.run_many(caps, oo)
    tims = []
    with wm.Batch(n_streams=n_streams, contexts=1, max_push_bytes=2 * n, **flags_to_kwargs(flags)) as b:
        for s in range(n_streams):
            b.stage(s, caps[s])
        b.run_resident(2 * n, 1, on_push=lambda f, c, recs, tm: tims.append(tm), want_lines=False)
        got = _batch_texts(b)
        assert ["".join(got.get(s, [])) for s in range(n_streams)] == want
        b.run_resident(2 * n, 1, on_push=lambda f, c, recs, tm: tims.append(tm), want_lines=False)
        got2 = _batch_texts(b)
    picks = list(range(0, n_streams, 8))
    want2 = oracle.run_many([caps[s] for s in picks], oo, passes=2)
    assert ["".join(got2.get(s, [])) for s in picks] == want2
    assert sum(len(w) for w in want) > 1000 and all(t["warnings"] == 0 for t in tims)


def test_c3_configuration_in_the_product_configuration(wm, oracle):
    """BASELINE configs[2] (4.0 MS/s, -d 5 -s, S1 + T1 + C1 concurrently, 2^22 IQ samples) without debug views: whole and in
    eight ragged pushes -- this capture lists more than a fifth of its tiles, so the eight-push run goes on demand ->
    paused, and the text is the oracle's either way."""
    flags = ["-d", "5", "-s", "-v"]
    cu8 = wm.synth_capture(seed=20260, n_samples=1 << 22, fs_khz=4000, kinds=15, frames_per_s=60.0, amplitude=60.0,
                           t1c1_center_khz=325.0, s1_center_khz=-325.0)[0]
    ref = oracle.run(cu8, flags_to_oracle_opts(oracle, flags))
    kw = dict(decimation=5, simultaneous=True, show_algorithm=True, keep_taps=False)
    with wm.Receiver(n_streams=1, max_push_bytes=cu8.size, **kw) as rx:
        assert rx.run(cu8)[0] == ref["text"]
        assert rx.timing()["rssi_mode"] in (wm.RSSI_ON_DEMAND, wm.RSSI_FELL_BACK)
    modes, text = [], []
    with wm.Receiver(n_streams=1, max_push_bytes=1 << 20, **kw) as rx:
        for off in range(0, cu8.size, 1 << 20):
            text.append(rx.push([cu8[off:off + (1 << 20)]]))
            modes.append(rx.timing()["rssi_mode"])
    assert "".join(text) == ref["text"]
    assert modes[0] in (wm.RSSI_ON_DEMAND, wm.RSSI_FELL_BACK) and wm.RSSI_PAUSED in modes, modes


def test_rssi_on_demand_goes_dense_pauses_and_comes_back(wm, oracle):
    """The state machine of RSSI on demand over 44 pushes of a stream whose bursts cover most of its tiles: on demand ->
    (more than a fifth of the tiles listed) sixteen pushes on the full pass -> on demand again ..., the RSSI filter's state
    handed over exactly each way.  wmbus_timing.rssi_mode says which path a push took, so a regression that silently
    disabled on demand, or never left the pause, fails here although the text would still be right.  A stretch of exact
    silence in the middle of the traffic cannot be proven by a tile computed on its own: with the pause switched off
    (rssi_dense_pm = 1000) the push that holds it must take the full pass (FELL_BACK, slow_path) -- and print the same text."""
    push, n_push, tiles_per_push = 1 << 16, 44, 17                    # 32768 IQ samples = 16384 decimated = 17 tiles of 976 per push
    cu8 = wm.synth_capture(seed=515, n_samples=n_push * push // 2, kinds=15, frames_per_s=400.0, amplitude=50.0)[0].copy()
    k_silent = 20
    cu8[k_silent * push + push // 4: k_silent * push + push // 2] = 128         # exact zero input, signal on both sides
    want = oracle.run(cu8, flags_to_oracle_opts(oracle, ["-v"]))["text"]
    assert len(want.splitlines()) > 100
    OD, PA, FB = wm.RSSI_ON_DEMAND, wm.RSSI_PAUSED, wm.RSSI_FELL_BACK

    def run(**kw):
        text, tims = [], []
        with wm.Receiver(n_streams=1, max_push_bytes=push, keep_taps=False, **kw) as rx:
            for k in range(n_push):
                text.append(rx.push([cu8[k * push:(k + 1) * push]]))
                tims.append(rx.timing())
        return "".join(text), tims

    text, tims = run()
    assert text == want
    modes = [t["rssi_mode"] for t in tims]
    pause, periods = 0, 0
    for k, t in enumerate(tims):                                      # the rule of wait_gpu (wm_api.hip), replayed on what the pushes reported
        if pause:
            assert t["rssi_mode"] == PA and t["rssi_tiles"] == 0 and t["rssi_ms"] == 0.0, (k, modes)
            pause -= 1
        else:
            assert t["rssi_mode"] in (OD, FB) and t["rssi_tiles"] > 0, (k, modes)
            assert (t["rssi_mode"] == FB) == bool(t["slow_path"]) or os.environ.get("WMBUS_TEST_ROUNDS_ON_HOST") == "1", (k, modes)
            if t["rssi_tiles"] * 1000 > 200 * tiles_per_push:
                pause, periods = 16, periods + 1
    assert modes[0] == OD and modes[1:17] == [PA] * 16 and modes[17] in (OD, FB)      # dense from the first push on
    assert periods >= 2                                               # ... and it came back and went again

    text, tims = run(rssi_dense_pm=1000)                              # never pause: every push on demand
    assert text == want
    assert all(t["rssi_mode"] in (OD, FB) and t["rssi_tiles"] > 0 for t in tims)


def test_rssi_on_demand_falls_back_for_a_telegram_right_behind_exact_silence(wm, oracle):
    """A telegram whose preamble begins in exact silence: the tile that holds its access code is listed, and the lanes of that
    tile whose warm-up lies in the silence cannot prove their start (lower trajectory 0, upper one still above it) -- THAT push
    must take the full pass (rssi_mode FELL_BACK, slow_path), every other push stays on demand, the text is the oracle's."""
    push, n_push = 1 << 16, 24                                        # 16384 decimated samples = 17 tiles per push
    cu8, frames = wm.synth_capture(seed=909, n_samples=n_push * push // 2, kinds=wm.T1 | wm.C1A | wm.C1B, frames_per_s=25.0, amplitude=50.0)
    cu8 = cu8.copy()
    pick = None
    for f in frames:                                                  # a frame whose access code (~384 decimated samples in) sits well inside a tile
        F = f["start"] // 2                                           # decimated sample of the frame's first chip
        k, p = divmod(F + 384, push // 4)
        if f["complete"] and 2 <= k < n_push - 1 and 2500 < p < push // 4 - 6000 and 400 < p % 976 < 900:
            pick = (f, F, k)
            break
    assert pick is not None
    f, F, k_silent = pick
    cu8[2 * 2 * (F - 2000): 2 * 2 * (F + 160)] = 128                  # exact zero input up to twenty chips into the preamble (the sync word stays)
    want = oracle.run(cu8, flags_to_oracle_opts(oracle, ["-v"]))["text"]
    assert f["telegram"].hex() in want                                # the telegram behind the silence is still received
    text, tims = [], []
    with wm.Receiver(n_streams=1, max_push_bytes=push, keep_taps=False, rssi_dense_pm=1000) as rx:
        for k in range(n_push):
            text.append(rx.push([cu8[k * push:(k + 1) * push]]))
            tims.append(rx.timing())
    assert "".join(text) == want
    modes = [t["rssi_mode"] for t in tims]
    assert modes[k_silent] == wm.RSSI_FELL_BACK and tims[k_silent]["slow_path"] == 1, (k_silent, modes)
    assert sum(m == wm.RSSI_ON_DEMAND for m in modes) >= n_push - 3, modes


@pytest.mark.parametrize("tune", [dict(k1_tiles_per_block=3), dict(k1_tiles_per_block=1, k1_small_tile=True), dict(k1_tiles_per_block=4, k1_small_tile=True), dict(clock_waves=1), dict(clock_waves=4)],
                         ids=["tpb3", "tpb1-small", "tpb4-small", "clock-one-wave", "clock-systolic"])
def test_tuning_fields_change_speed_not_output(wm, oracle, samples, tune):
    """The launch-structure knobs of round 5 (k1_tiles_per_block / k1_small_tile: how the demodulation kernel's first pass cuts a
    push into blocks, with the next tile's input prefetched) and round 6 (clock_waves: the clock-recovery cascade on one wave
    or on the four waves of a block) against the oracle: the bundled capture whole and in ragged pushes,
    and 70 synthetic captures (one whole wave + a ragged one) with warm-ups short enough that every kind of re-run list is long
    -- in two pushes, so that carried state crosses them."""
    cu8 = samples["samples2"][: samples["samples2"].size // 4096 * 4096]
    want = oracle.run(cu8, flags_to_oracle_opts(oracle, ["-v"]))["text"]
    for push in (cu8.size, 4096 * 37):
        with wm.Receiver(n_streams=1, max_push_bytes=push, keep_taps=False, **tune) as rx:
            assert rx.run(cu8, push_bytes=push)[0] == want, push
    n = 1 << 19
    caps = [wm.synth_capture(seed=8800 + s, n_samples=n, kinds=15, frames_per_s=150.0, amplitude=40.0)[0] for s in range(70)]
    wants = oracle.run_many(caps, flags_to_oracle_opts(oracle, ["-v"]))
    with wm.Receiver(n_streams=70, max_push_bytes=n, keep_taps=False, seg_len=8192, rla_seg_len=2048, warmup_t1c1=2048, warmup_s1=4096, **tune) as rx:
        text = [""] * 70
        for off in (0, n):
            rx.push([c[off:off + n] for c in caps])
            for ln in rx.lines():
                text[ln["stream"]] += ln["text"]
            tm = rx.timing()
            assert tm["clock_reruns"] > 0 and tm["rla_reruns"] > 0
    assert text == wants


def _free_device_memory():
    """hipMemGetInfo of the current device, through the HIP runtime the library has already brought into this process."""
    import ctypes
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


@pytest.mark.parametrize("cfg", [dict(keep_taps=False), dict(keep_taps=True), dict(input_rate_hz=2_400_000, input_format=2), dict(input_format=1),
                                 dict(input_windows=2), dict(prefilter=1)],
                         ids=["rssi-on-demand", "keep-taps", "resample-cs16", "convert-cs8", "two-windows", "polyphase"])
def test_open_close_returns_device_memory(wm, cfg):
    """wmbus_close (and nothing else) gives back what wmbus_open took: the six configurations together reach every conditional
    allocation of a context (d_rs_* / d_plans; all of K0; K0 without taps or history; the second input window and its copy
    stream; the polyphase kernel's context).  One open / push of silence / collect / close lets the runtime settle; sixteen more
    such cycles must not cost more free device memory than ONE input window, n_streams x max_push_bytes = 128 KiB: a condition,
    not a measurement -- the runtime may keep small pools of its own, while any push-sized buffer leaked once per cycle would
    exceed it sixteen times over (smaller buffers are covered by there being a single free path).  The commit before the
    single free path passes unchanged: 0 bytes lost in each of the six configurations, twice.  With it: 0 bytes in all six in one
    run; in another, 2 097 152 bytes (one 2 MiB block) in `keep-taps` and 0 in the other five -- over the limit, not yet explained."""
    assert wm.FMT_CS16 == 2 and wm.FMT_CS8 == 1
    n_streams, push = 2, 65536
    silence = np.full(push, 0 if "input_format" in cfg else 128, np.uint8)

    def cycle():
        with wm.Receiver(n_streams=n_streams, max_push_bytes=push, **cfg) as rx:
            rx.push([silence] * n_streams)

    cycle()
    before = _free_device_memory()
    for _ in range(16):
        cycle()
    lost = before - _free_device_memory()
    print(f"free device memory lost over 16 open / close cycles: {lost} bytes")
    assert lost <= n_streams * push, lost
