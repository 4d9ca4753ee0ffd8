"""Batch lanes on the GPU (wm_batch.h): contexts that share a hardware queue are driven as one lane -- one stream, the framer and
burst kernels of both in ONE launch (gridDim.z = 2, wm_k_pair.h).  Every case forces its lane count with WMBUS_BATCH_LANES, whatever
the host presets, asserts through wmbus_batch_lane_stats that launches really were paired, and holds every capture's lines against
the same batch with a lane per context (the launches of before) and against the oracle.

Inputs: kinds = 15 at 200 frames/s, 3 pushes of 2^15 IQ samples per capture, clock segments of 4096 and run-length segments of 1024
decimated samples: every push has four clock and sixteen run-length segments per row, so list rounds and carries run."""
import os

import pytest

from cases import flags_to_oracle_opts
from lanes import LANE_N_PUSH, LANE_PUSH, LANE_SEGS, conserved, lane_caps, lane_run

pytestmark = pytest.mark.gpu

PUSH, N_PUSH, SEGS = LANE_PUSH, LANE_N_PUSH, LANE_SEGS


@pytest.fixture(scope="module")
def caps(wm):
    """192 captures of three pushes (read-only: every case takes a prefix)."""
    return lane_caps(wm, 192)


@pytest.fixture(scope="module")
def want(caps, oracle):
    """The oracle's text: of every capture whole ("stream": a host-sourced run's three pushes together), of its first push alone, and
    of that push fed once, twice and three times ("resident": pass k of a resident run)."""
    opts, th = flags_to_oracle_opts(oracle, ["-v"]), min(32, os.cpu_count() or 1)
    first = [c[:PUSH] for c in caps[:128]]
    return {"stream": oracle.run_many(caps, opts, threads=th), "first": oracle.run_many(first, opts, threads=th),
            "resident": [oracle.run_many(first, opts, passes=k + 1, threads=th) for k in range(N_PUSH)]}


def run(wm, caps, S, contexts, lanes, resident, **kw):
    """One batch run under WMBUS_BATCH_LANES=lanes.  Returns (per capture: the text of every push, the lane statistics, the plan)."""
    r = lane_run(wm, caps, S, contexts, lanes, resident, push=PUSH, n_push=N_PUSH, input_windows=1 if resident else 2, **SEGS, **kw)
    return r.text, r.stats, r.plan


def both(wm, caps, S, contexts, lanes, resident, **kw):
    """The run in lanes and the same run with a lane per context; their lines must agree push for push, and the launches of the
    second are those of the first with every paired launch counted twice (lanes.py)."""
    text, stats, plan = run(wm, caps, S, contexts, lanes, resident, **kw)
    alone, stats1, plan1 = run(wm, caps, S, contexts, contexts, resident, **kw)
    assert plan1 == plan and stats1["lanes"] == contexts and stats1["paired"] == 0 and stats1["single"] > 0
    assert conserved(stats, stats1), (stats, stats1)
    assert text == alone
    assert sum(len(t) for per in text for t in per) > 1000 * S // 128       # the captures decode to something
    return text, stats, plan


def resident_matches(text, want, S):
    for k in range(N_PUSH):
        assert [text[s][k] for s in range(S)] == want["resident"][k][:S], f"pass {k + 1}"


def test_two_whole_wave_contexts_in_one_lane(wm, caps, want):
    """128 captures, 2 contexts, 1 lane, resident input as the benchmark has it: whole waves, the cooperative clock form in both."""
    text, stats, plan = both(wm, caps, 128, 2, 1, True)
    assert plan == [(0, 64), (64, 64)] and stats["lanes"] == 1 and stats["paired"] > 0
    resident_matches(text, want, 128)


def test_mates_of_different_clock_forms_and_grids(wm, caps, want):
    """130 captures = 64 + 66: the first mate loads cooperatively, the second lane by lane -- two different clock kernels, which leave
    singly -- and every other paired launch has two different grids: the blocks of the larger grid that lie outside the smaller
    context's return, every block inside it works on its own context."""
    text, stats, plan = both(wm, caps, 130, 2, 1, False)
    assert plan == [(0, 64), (64, 66)] and stats["lanes"] == 1 and stats["paired"] > 0 and stats["single"] > 0
    assert ["".join(t) for t in text] == want["stream"][:130]


def test_three_contexts_in_two_lanes(wm, caps, want):
    """192 captures, 3 contexts, 2 lanes: one pair and one context alone."""
    text, stats, plan = both(wm, caps, 192, 3, 2, False)
    assert plan == [(0, 64), (64, 64), (128, 64)] and stats["lanes"] == 2 and stats["paired"] > 0 and stats["single"] > 0
    assert ["".join(t) for t in text] == want["stream"][:192]


def test_rounds_on_the_host_in_a_lane(wm, caps, want):
    """rounds_on_host = 1: no hand-off round is enqueued unattended, every push of both mates is finished with the host in the loop
    (finish_slowly), on the lane's stream, while the mate's results wait."""
    text, stats, _plan = both(wm, caps, 128, 2, 1, True, rounds_on_host=1)
    assert stats["lanes"] == 1 and stats["paired"] > 0
    resident_matches(text, want, 128)


def test_a_mate_whose_source_ends_first_leaves_the_lane_to_the_other(wm, caps, want):
    """Host-sourced: the first context's source ends after one push, its mate's after three -- the mate goes on singly."""
    text, stats, _plan = both(wm, caps, 128, 2, 1, False, pushes_of={0: 1})
    assert stats["lanes"] == 1 and stats["paired"] > 0 and stats["single"] > 0
    assert [len(t) for t in text] == [1] * 64 + [3] * 64
    assert [t[0] for t in text[:64]] == want["first"][:64]
    assert ["".join(t) for t in text[64:]] == want["stream"][64:128]


def test_a_lane_per_context_is_the_launch_sequence_of_before(wm, caps, want):
    """WMBUS_BATCH_LANES >= contexts: a worker, a stream and plain launches per context -- no paired launch at all."""
    text, stats, plan = run(wm, caps, 128, 2, 2, True)
    assert plan == [(0, 64), (64, 64)] and stats == dict(lanes=2, paired=0, single=stats["single"]) and stats["single"] > 0
    resident_matches(text, want, 128)
    text8, stats8, _ = run(wm, caps, 128, 2, 8, True)
    assert stats8["lanes"] == 2 and stats8["paired"] == 0 and text8 == text
