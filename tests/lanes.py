"""Batch lanes in the GPU tests (TEST INFRASTRUCTURE, a plain module): open a wm.Batch with a forced lane count, drive it, keep everything
its sink was handed -- the whole line records (text, crc_ok, level / repair / quality / power dicts), every push's timing dict,
Batch.bursts -- and the lane statistics; and hold a run in lanes against the same run with a lane per context.

Launch conservation (lane_both): a paired launch carries exactly the two plain launches it replaces and nothing else appears or
vanishes, so 2 * paired + single of the lane run equals single of the lane-per-context run."""
import contextlib
import os

ENV = "WMBUS_BATCH_LANES"


@contextlib.contextmanager
def forced_lanes(n):
    """WMBUS_BATCH_LANES = n around a wm.Batch(...) open (the library reads it there and nowhere else); the old value comes back."""
    old = os.environ.get(ENV)
    os.environ[ENV] = str(n)
    try:
        yield
    finally:
        if old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = old


LANE_PUSH = 2 << 15            # bytes of a push of the lane tests: 2^15 IQ samples
LANE_N_PUSH = 3
LANE_SEGS = dict(seg_len=4096, rla_seg_len=1024)      # four clock and sixteen run-length segments per row and push: list rounds and carries run


def lane_caps(wm, n, first=0, fs_khz=1600, kinds=15, n_push=LANE_N_PUSH, offset_khz=0.0):
    """Captures first .. first + n - 1 of the lane tests (read-only): kinds = 15 at 200 frames/s, n_push pushes of 2^15 IQ samples; a
    pure function of the arguments, so every module that asks gets the same bytes.  offset_khz: T1/C1 that far above the centre and S1
    that far below, where -s looks for them."""
    out = [wm.synth_capture(seed=0x1A7E5 + i, n_samples=n_push * LANE_PUSH // 2, fs_khz=fs_khz, kinds=kinds, frames_per_s=200.0 if kinds else 0.0,
                             t1c1_center_khz=offset_khz, s1_center_khz=-offset_khz)[0]
           for i in range(first, first + n)]
    for c in out:
        assert c.size == n_push * LANE_PUSH
        c.setflags(write=False)
    return out


class LaneRun:
    """What one batch run delivered.  lines[s]: per push of capture s's context the line dicts of s; timing[first stream of a context]:
    the timing dict of every push; bursts: Batch.bursts; stats: Batch.lane_stats(); plan: [(first stream, captures)] per context."""

    def __init__(self, S):
        self.lines = [[] for _ in range(S)]
        self.timing, self.bursts, self.stats, self.plan, self.run_stats = {}, {}, None, None, None

    @property
    def text(self):
        """Per capture the text of every push (what test_gpu_lanes.py compares)."""
        return [["".join(ln["text"] for ln in push) for push in per] for per in self.lines]

    def whole_text(self, s):
        return "".join(ln["text"] for push in self.lines[s] for ln in push)


def conserved(lane_stats, alone_stats):
    """Each paired launch replaces exactly two plain ones."""
    return 2 * lane_stats["paired"] + lane_stats["single"] == alone_stats["single"]


def lane_run(wm, caps, S, contexts, lanes, resident=False, *, push, n_push=1, pushes_of=None, sizes_of=None, after=None, **kw):
    """One batch run of captures caps[:S] under WMBUS_BATCH_LANES = lanes; `kw` goes to wm.Batch.
    resident: caps[s][:push] is staged and every context makes n_push passes over it.
    Host-sourced otherwise (kw needs input_windows = 2): every context pushes its captures front to back -- n_push pushes of `push`
    bytes, or pushes_of[first stream] of them, or the byte counts sizes_of[first stream] (each a multiple of 4096, at most `push`).
    after(batch): called behind the run while the batch is still open (what is read through Batch.contexts: locks, surveys)."""
    with forced_lanes(lanes):
        b = wm.Batch(n_streams=S, contexts=contexts, max_push_bytes=push, **kw)
    out = LaneRun(S)
    with b:
        out.plan = [(first, n) for _rx, first, n in b.contexts]

        def on_push(first, n, lines, tm):
            assert tm["warnings"] == 0
            out.timing.setdefault(first, []).append(tm)
            for s in range(first, first + n):
                out.lines[s].append([])
            for ln in lines:
                assert first <= ln["stream"] < first + n
                out.lines[ln["stream"]][-1].append(ln)
        if resident:
            for s in range(S):
                b.stage(s, caps[s][:push])
            st = b.run_resident(push, n_push, on_push)
            assert st["pushes"] == len(out.plan) * n_push
        else:
            sizes = {first: list((sizes_of or {}).get(first, [push] * (pushes_of or {}).get(first, n_push))) for first, _n in out.plan}
            done = {first: 0 for first, _n in out.plan}
            at = {first: 0 for first, _n in out.plan}

            def fill(first, n, slab):
                k = done[first]
                if k == len(sizes[first]):
                    return 0
                done[first] = k + 1
                nb, off = sizes[first][k], at[first]
                at[first] = off + nb
                for j in range(n):
                    assert off + nb <= caps[first + j].size
                    slab[j, :nb] = caps[first + j][off:off + nb]
                return nb
            st = b.run_from(fill, on_push)
            assert st["pushes"] == sum(len(v) for v in sizes.values())
        out.run_stats, out.stats, out.bursts = st, b.lane_stats(), {k: list(v) for k, v in b.bursts.items()}
        if after:
            after(b)
    return out


def one_lane(wm, caps, S, resident=False, **kw):
    """The lane leg of a stage's batch test: caps[:S] in two contexts that share ONE lane, held against the lane-per-context run; the
    stage's own reference stays the caller's.  Returns the lane run."""
    got, _alone = lane_both(wm, caps, S, 2, 1, resident, **kw)
    assert len(got.plan) == 2 and got.stats["lanes"] == 1 and got.stats["paired"] > 0
    return got


def lane_both(wm, caps, S, contexts, lanes, resident=False, **kw):
    """The run in lanes and the same run with a lane per context: the same plan, no paired launch in the second, launch conservation,
    and every record of every push equal.  Returns (the lane run, the lane-per-context run)."""
    got = lane_run(wm, caps, S, contexts, lanes, resident, **kw)
    alone = lane_run(wm, caps, S, contexts, contexts, resident, **kw)
    assert alone.plan == got.plan and alone.stats["lanes"] == contexts and alone.stats["paired"] == 0 and alone.stats["single"] > 0
    assert got.text == alone.text
    assert got.lines == alone.lines and got.bursts == alone.bursts
    assert conserved(got.stats, alone.stats), (got.stats, alone.stats)
    return got, alone
