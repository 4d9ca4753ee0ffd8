"""Two mates of one batch lane that do NOT record the same list (wm_launch.h, wm_lane_merge.h): host-sourced runs (input_windows = 2)
of two contexts in one lane whose pushes differ in size, in RSSI mode, or in whether they reach the pipeline at all.  The merge then
meets lists of which one lacks launches the other has -- the branch where a pairable head "holds on while the other list catches up"
-- and pushes whose mate has nothing in flight.  Every case holds every capture's lines against the oracle on the bytes that capture
was fed, concatenated, and, push for push, against the same batch with a lane per context (lanes.py: launch conservation too).

  small mate      context 0 pushes 2^15 samples three times, context 1 2^12 samples eight times: one clock segment per push, so its
                  clock kernel has no list rounds (g.nseg > 1 in enqueue_front_impl) while its mate's has five
  out of step     big, small, big against small, big, small
  RSSI paused     rssi_dense_pm = 300: a context whose push lists more than 300 per mille of its tiles takes the full RSSI pass for
                  sixteen pushes (rs_pause) -- no k3_spans and no RSSI relaunch in its back, the tile hand-off rounds in its front --
                  while its mate, fed noise, stays on demand
  no block        a resampling context (2.048 MS/s -> 1.6 MS/s, 25 / 32) whose first push of 4096 raw bytes is 3200 resampled ones:
                  g.M == 0, the front is the input stage alone and the back is empty, beside a mate's full push"""
import os

import numpy as np
import pytest

import resample_ref as RR
from cases import flags_to_oracle_opts
from lanes import LANE_PUSH, LANE_SEGS, lane_both, lane_caps

pytestmark = pytest.mark.gpu

BIG, SMALL = LANE_PUSH, 2 << 12                     # bytes: 2^15 and 2^12 IQ samples


@pytest.fixture(scope="module")
def caps(wm):
    return lane_caps(wm, 6)


def oracle_text(oracle, fed):
    return oracle.run_many(fed, flags_to_oracle_opts(oracle, ["-v"]), threads=min(32, os.cpu_count() or 1))


def mates(wm, oracle, caps, sizes_of, push=BIG, feed=None, **kw):
    """Captures 0-2 in context 0 and 3-5 in context 1, one lane, the byte counts sizes_of[first stream]; lines against the oracle on what
    every capture was fed (feed(capture bytes): what the pipeline gets of them, default: the bytes) and against the lane-per-context run."""
    got, _alone = lane_both(wm, caps, 6, 2, 1, push=push, sizes_of=sizes_of, input_windows=2, **LANE_SEGS, **kw)
    assert got.plan == [(0, 3), (3, 3)] and got.stats["lanes"] == 1 and got.stats["paired"] > 0
    fed = [caps[s][:sum(sizes_of[0 if s < 3 else 3])] for s in range(6)]
    want = oracle_text(oracle, [feed(f) for f in fed] if feed else fed)
    assert [got.whole_text(s) for s in range(6)] == want
    assert [len(per) for per in got.lines] == [len(sizes_of[0])] * 3 + [len(sizes_of[3])] * 3
    return got, want


def test_one_mate_pushes_small(wm, oracle, caps):
    got, want = mates(wm, oracle, caps, {0: [BIG] * 3, 3: [SMALL] * 8})
    assert got.stats["single"] > 0
    assert any(want[:3]) and any(want[3:])
    assert all(tm["clock_round"] == [0, 0, 0, 0] for tm in got.timing[3])      # one clock segment: no list round ran for the small mate


def test_alternating_sizes_out_of_step(wm, oracle, caps):
    got, want = mates(wm, oracle, caps, {0: [BIG, SMALL, BIG], 3: [SMALL, BIG, SMALL]})
    assert got.stats["single"] > 0
    assert any(want[:3]) and any(want[3:])


def test_a_mate_on_the_full_rssi_pass(wm, oracle):
    """Context 0: captures whose first telegram begins inside the first push (lanes.py's captures 3, 6 and 7: samples 4598, 6719, 6966);
    context 1: noise.  20 pushes of 2^13 samples: context 0 lists 7 of its 3 x 5 tiles in push 0, is paused for pushes 1 .. 16 and comes
    back to on demand with push 17 (6 tiles: paused again); context 1 lists its captures' last tiles (once a fourth tile: a chance access code in the noise) and stays on demand.

    The threshold is 300 per mille and not 1: k3_spans ALWAYS lists the last tile of every capture (it carries the filter's state into
    the next push), so a push of 2^13 samples -- 4096 decimated ones, five tiles a capture -- lists 200 per mille at least, and with
    rssi_dense_pm = 1 no context of such pushes can stay on demand, whatever it is fed: measured with noise of sigma 3, with +-1 LSB,
    with the constant bytes 128 and 127/128, three tiles listed and the pause taken every time.  Between 200 (the mate: 3 of 15) and
    400 (context 0: 6 of 15) both mates are where this case wants them; 300 also holds if a capture had four tiles."""
    caps = [lane_caps(wm, 1, first=i, n_push=5)[0] for i in (3, 6, 7)] + lane_caps(wm, 3, first=192, kinds=0, n_push=5)
    n, push = 20, 2 << 13
    got, want = mates(wm, oracle, caps, {0: [push] * n, 3: [push] * n}, push=push, rssi_dense_pm=300)
    mode = {first: [tm["rssi_mode"] for tm in got.timing[first]] for first in (0, 3)}
    print("rssi_mode per push:", mode, "tiles listed:", {first: [tm["rssi_tiles"] for tm in got.timing[first]] for first in (0, 3)})
    # the mate: the last tile of each of its three captures at least, and never more than the threshold's 300 per mille of 3 x 5 tiles
    assert all(3 <= tm["rssi_tiles"] and 1000 * tm["rssi_tiles"] <= 300 * 3 * 5 for tm in got.timing[3])
    assert mode[0][1] == wm.RSSI_PAUSED
    assert mode[3] == [wm.RSSI_ON_DEMAND] * n
    assert mode[0][0] == wm.RSSI_ON_DEMAND and mode[0][1:17] == [wm.RSSI_PAUSED] * 16 and mode[0][17] == wm.RSSI_ON_DEMAND
    assert all(want[:3]) and not any(want[3:])


def test_a_push_that_completes_no_block_for_one_mate(wm, oracle):
    """2.048 MS/s -> 1.6 MS/s is 25 / 32: 4096 raw bytes are 2048 samples in and 1600 out, 3200 bytes and no whole block (g.M == 0)."""
    fin = 2048000
    L, M, _T, taps = wm.resampler_design(fin, 1600000)
    caps = lane_caps(wm, 6, fs_khz=2048)
    assert RR.resample(caps[0][:4096], L, M, taps).size == 3200 and RR.pipeline_bytes(caps[0][:4096], L, M, taps).size == 0
    sizes = {0: [4096, BIG, BIG, 3 * BIG - 4096 - 2 * BIG], 3: [BIG] * 3}
    got, want = mates(wm, oracle, caps, sizes, feed=lambda raw: RR.pipeline_bytes(np.asarray(raw), L, M, taps), input_rate_hz=fin)
    assert got.timing[0][0]["input_bytes_out"] == 3 * 3200 and all(per[0] == [] for per in got.lines[:3])      # resampled, not yet a block
    assert got.timing[3][0]["input_bytes_out"] == 3 * 2 * (BIG // 2 * L // M)
    assert any(want[:3]) and any(want[3:])
