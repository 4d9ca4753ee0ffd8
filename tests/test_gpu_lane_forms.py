"""Every paired kernel form of a batch lane (wm_k_pair.h) at the smallest shapes that launch it, and every reference switch that changes
the sequence of operations a push records (wm_launch.h): two contexts in ONE lane, host-sourced, 3 pushes of 2^15 IQ samples, clock
segments of 4096 and run-length segments of 1024 decimated samples (list rounds and carries run; lanes.py has the inputs, they are
test_gpu_lanes.py's).  Every case asserts: the lines of every capture equal the CPU oracle's under the matching reference switches;
they equal, push for push, the same batch with a lane per context (and 2 * paired + single launches of the lane run are the launches
of that one); launches were paired.

Which paired clock kernel a case launches follows from fr_launch (wm_api.hip): DC = remove_dc, COOP = whole waves of 64 captures in
the context, and two mates' first passes leave as one launch only where both pick the same kernel:
  3+3                k2_clock_sys_pair<false, false>, k2_clock_sys_list_pair<false>
  64+64 remove_dc    k2_clock_sys_pair<true, true>, k2_clock_sys_list_pair<true>
  3+3 remove_dc      k2_clock_sys_pair<true, false>, k2_clock_sys_list_pair<true>
  3+2                <false, false> with two different grids in every paired launch (k3_scan's grid.x, the framers', the list rounds')
  clock_waves=1      the one-wave clock kernels have no paired form: they leave singly between the paired run-length launches
(<false, true> is test_gpu_lanes.py's 64+64.)  That the CLOCK launches pair, and not only the run-length and burst ones, is asserted
by difference: the same run with clock_waves = 1 has at least one paired launch per pair of pushes fewer."""
import os

import pytest

from cases import flags_to_kwargs, flags_to_oracle_opts
from lanes import LANE_N_PUSH, LANE_PUSH, LANE_SEGS, lane_both, lane_caps, lane_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def caps(wm):
    return {1600: lane_caps(wm, 128), 2400: lane_caps(wm, 6, fs_khz=2400), "-s": lane_caps(wm, 6, offset_khz=325.0)}


@pytest.fixture(scope="module")
def want(caps, oracle):
    """The oracle's text of captures [0, n) under reference switches `flags`: computed once per (switches, rate), shared, left unchanged."""
    memo = {}

    def text(flags, n, fs=1600):
        key = (tuple(flags), fs)
        if len(memo.get(key, ())) < n:
            memo[key] = oracle.run_many(caps[fs][:n], flags_to_oracle_opts(oracle, flags), threads=min(32, os.cpu_count() or 1))
        return memo[key][:n]
    return text


def one_lane(wm, caps, S, **kw):
    """`S` captures in two contexts and one lane, against the lane-per-context run."""
    got, _alone = lane_both(wm, caps, S, 2, 1, push=LANE_PUSH, n_push=LANE_N_PUSH, input_windows=2, **LANE_SEGS, **kw)
    assert got.stats["lanes"] == 1 and got.stats["paired"] > 0
    assert all(len(per) == LANE_N_PUSH for per in got.lines)
    return got


def clock_launches_pair(wm, caps, S, got, **kw):
    """The same data with the one-wave clock form, whose launches cannot pair: at least the first pass of every pair of pushes is missing
    from the paired count."""
    plain = lane_run(wm, caps, S, 2, 1, push=LANE_PUSH, n_push=LANE_N_PUSH, input_windows=2, clock_waves=1, **LANE_SEGS, **kw)
    assert plain.text == got.text
    print("paired launches:", got.stats["paired"], "with the one-wave clock form:", plain.stats["paired"])
    assert got.stats["paired"] - plain.stats["paired"] >= LANE_N_PUSH


FORMS = {"3+3": (6, [(0, 3), (3, 3)], ["-v"]), "64+64-dc": (128, [(0, 64), (64, 64)], ["-o", "-v"]),
         "3+3-dc": (6, [(0, 3), (3, 3)], ["-o", "-v"]), "3+2": (5, [(0, 3), (3, 2)], ["-v"])}


@pytest.mark.parametrize("form", list(FORMS))
def test_paired_clock_forms(wm, caps, want, form):
    S, plan, flags = FORMS[form]
    kw = flags_to_kwargs(flags)
    got = one_lane(wm, caps[1600], S, **kw)
    assert got.plan == plan
    assert [got.whole_text(s) for s in range(S)] == want(flags, S)
    assert all(got.whole_text(s) for s in range(S))                      # every capture decodes to something
    clock_launches_pair(wm, caps[1600], S, got, **kw)


def test_one_wave_clock_kernels_leave_singly_between_paired_launches(wm, caps, want):
    got = one_lane(wm, caps[1600], 6, clock_waves=1)
    assert got.stats["single"] > 0
    assert [got.whole_text(s) for s in range(6)] == want(["-v"], 6)


SWITCHES = {"-r 0": ["-r", "0", "-v"], "-t 0": ["-t", "0", "-v"], "-p S": ["-p", "S", "-v"], "-p T": ["-p", "T", "-v"], "-a": ["-a", "-v"], "-s": ["-s", "-v"]}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_switches_that_change_the_recorded_sequence(wm, caps, want, name):
    """-r 0: no run-length framer, fr_carry's recorded device-to-device copy; -t 0, -p S, -p T, -a, -s: RSSI at every sample (no
    k3_spans, the tile hand-off rounds in the front) and other framer lists."""
    flags = SWITCHES[name]
    fs = "-s" if name == "-s" else 1600                                # -s: the captures with T1/C1 at +325 kHz and S1 at -325 kHz
    got = one_lane(wm, caps[fs], 6, **flags_to_kwargs(flags))
    text = [got.whole_text(s) for s in range(6)]
    assert text == want(flags, 6, fs=fs)
    assert sum(1 for t in text[:3] if t) and sum(1 for t in text[3:] if t)      # lines in both contexts


def test_rssi_at_every_sample(wm, caps, want):
    """keep_taps = True: the debug views' configuration, no k3_spans and no RSSI relaunch in the back."""
    got = one_lane(wm, caps[1600], 6, keep_taps=True)
    assert [got.whole_text(s) for s in range(6)] == want(["-v"], 6)
    assert all(tm["rssi_mode"] == wm.RSSI_EVERY_SAMPLE for per in got.timing.values() for tm in per)


def test_decimation_3(wm, caps, want):
    """-d 3 on captures synthesised at 2400 kHz."""
    got = one_lane(wm, caps[2400], 6, decimation=3)
    text = [got.whole_text(s) for s in range(6)]
    assert text == want(["-d", "3", "-v"], 6, fs=2400) and all(text)


def test_tolerance_mode(wm, caps):
    """cfg.tolerance_mode (no early hand-over of the K1 turn: one demodulation launch inside the turn).  The oracle has no such mode
    -- its soft symbols are the exact ones -- so this case is held against the lane-per-context run only."""
    got = one_lane(wm, caps[1600], 6, tolerance_mode=1)
    assert all(got.whole_text(s) for s in range(6))
