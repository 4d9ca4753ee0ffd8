"""The COMPILED run-length kernel on designed captures, and the kernel's integer divisions over their whole domain on the device.

Slicer bits cannot be handed to the library, but they can be read back: every capture here is modulated so that its slicer
bits are what the case needs (telegram_ref.modulate_runs), the bits the GPU reads back must be the oracle's, and those bits
and the RSSI tap go through the per-sample restatement tests/rla_ref.py, push by push with the state carried, which must give
what wmbus_read_chips gives: positions, values, markers and RSSI bytes.  The first half of this file needs no GPU: it holds
each case to what it is for (rla_ref's events on the oracle's bits), so a case that has drifted away from its purpose fails
here and not silently.  tests/README.md, "The run-length framer's input space"."""
import ctypes

import numpy as np
import pytest

import rla_ref
import telegram_ref as TR
from cases import flags_to_kwargs, flags_to_oracle_opts
from lanes import one_lane

BLOCK = 4096
PUSH = 1 << 17                                            # bytes of a push of the d = 2 cases: 2^15 decimated samples, 32 segments
SEGS = dict(seg_len=4096, rla_seg_len=1024)
LOOKBACKS = (32, 256)
RAGGED_BLOCKS = 16                                        # blocks of the largest push of the -d 13 / -d 15 schedules

# Exact silence slices to raw ones; the deglitched run it makes also holds what the noise in front and the preamble behind
# contribute.  The lengths (decimated samples) were tuned on the CPU against rla_ref's events, which the precondition below
# asserts: T1/C1 runs of exactly 65535, 65536 and 65537 samples (the first division's dividend beyond 2^24, where wm_udiv
# must take the integer divide), and runs that give 8191, 8192 and 8193 chips (WM_RLA_RUN_LIMIT and its neighbours).
SILENCE_SAMPLES = (65542, 65544, 65545)
SILENCE_CHIPS = (63153, 64995, 64907)
WANT_RUNS = (65535, 65536, 65537)
WANT_CHIPS = (8191, 8192, 8193)


def runs_parts(noisy):
    """Runs of 4..60 decimated samples, each length twenty times with the next one (so that the edges wander through the
    words); faster ones, which reset both framers; then, per chain, runs of n = 1..25 chips, each behind a stretch that resets
    the framer and a few chips of nominal length (a tracker left alone follows slowly growing runs and n stays at 1 or 2)."""
    parts = [("noise", 1500)]
    for L in range(4, 61):
        parts.append(("runs", [L, L + 1] * 20, 1, noisy))
    parts += [("runs", [2, 3] * 300, 1, noisy), ("runs", [3, 4] * 300, 1, noisy), ("noise", 1500)]
    for pulse, gap in ((4, 13), (5, 14)):                                                     # pulses too short for T1/C1, either level (periods 17 and 19)
        parts += [("runs", [pulse, gap] * 100, 1, noisy), ("runs", [pulse, gap] * 100, 0, noisy)]
    parts += [("runs", [L, L + 1] * 100, 1, noisy) for L in (9, 10, 11, 12)]                 # runs of about half an S1 bit
    for spc in (8, 24):
        for run in range(spc, 25 * spc + 1, spc // 2):                                        # every n whatever the tracker has made of the chips in front
            parts.append(("runs", [2] * 8 + [spc] * 8 + [run, spc, spc], 1, noisy))
    return parts


def silence_parts(lengths):
    parts = [("noise", 1500)]
    for i, n in enumerate(lengths):
        parts += [("silence", n, 127 + i % 2), ("chips", "C1A", TR.preamble("C1A") + [0, 1] * 8, True), ("noise", 700)]
    return parts


CASES = {
    "runs, noisy": lambda: TR.modulate_runs(runs_parts(True), seed=11, block=PUSH),
    "runs, clean": lambda: TR.modulate_runs(runs_parts(False), seed=12, block=PUSH),
    "noise alone": lambda: TR.modulate_runs([("noise", 3 * (PUSH // 4))], seed=13, block=PUSH),
    "silences, samples": lambda: TR.modulate_runs(silence_parts(SILENCE_SAMPLES), seed=14, block=PUSH),
    "silences, chips": lambda: TR.modulate_runs(silence_parts(SILENCE_CHIPS), seed=15, block=PUSH),
}
_case = {}


def case(oracle, name, flags=("-v",)):
    """(cu8, the oracle's taps, rla_ref over the oracle's bits per chain), once per session"""
    if name not in _case:
        cu8 = CASES[name]()
        assert cu8.size % PUSH == 0 and cu8.size <= 1 << 20              # at most 2^19 input samples
        cu8.setflags(write=False)
        o = oracle.run(cu8, flags_to_oracle_opts(oracle, list(flags)), taps=True)
        ref = [rla_ref.run(ch, o["bit"][ch], rssi=o["rssi"][ch].astype(np.uint32)) for ch in (0, 1)]
        _case[name] = (cu8, o, ref)
    return _case[name]


def edge_ks(events):
    chip = {e["sample"] % 64 for e in events if e["kind"] == rla_ref.CHIPS}
    reset = {e["sample"] % 64 for e in events if e["kind"] != rla_ref.CHIPS}
    return chip, reset


# ---- the ragged pushes of -d 13 and -d 15 ----------------------------------------------------------------------------------------
_ragged = {}


def ragged_case(wm, oracle, d):
    """A synthetic capture at d x 800 kHz and a schedule of pushes (whole 4096-byte blocks, RAGGED_BLOCKS at most) whose
    decimated lengths end 4 samples into a 64-sample word as often as the decimator's carried phase allows: the first is 11
    blocks at -d 13 (1732 = 27 x 64 + 4 samples) and 8 blocks at -d 15 (1092 = 17 x 64 + 4); the later ones are enumerated
    from the oracle's sample count after every block, since the phase carried into a push decides between 4 and 5.  At -d 15
    three pushes of 8 blocks in a row end at 4 (phases 0, 4, 8), then 6 blocks bring the phase back to 0; at -d 13 only a push
    from phase 0 does, so pushes of 11 and of 2 blocks alternate.
    Why 4 alone: a push is a whole number of blocks of 2048 input samples, so its length is floor or ceil of 2048 nb / d, and
    2048 nb / d modulo 64 runs through d values at most (13 blocks at -d 13 and 15 at -d 15 are exactly 2048 samples).  At
    -d 13 these are 29.5, 59.1, 24.6, 54.2, 19.7, 49.2, 14.8, 44.3, 9.8, 39.4, 4.9, 34.5, 0 and at -d 15 multiples of
    8.53: of the residues below five only 4 (and 0) can be reached, and no decimation 1..16 reaches 1, 2 or 3.  Those are
    the emulator's (tests/test_rla_space_emulated.py::test_ragged_pushes)."""
    if d not in _ragged:
        cu8 = wm.synth_capture(seed=7300 + d, n_samples=1 << 18, fs_khz=800 * d, kinds=15, frames_per_s=400.0, amplitude=60.0)[0]
        cu8 = cu8[: cu8.size // BLOCK * BLOCK]
        cu8.setflags(write=False)
        flags = ["-v", "-d", str(d)]
        o = oracle.run(cu8, flags_to_oracle_opts(oracle, flags), taps=True)
        L = oracle.lib()
        ctx = L.wmo_new(ctypes.byref(flags_to_oracle_opts(oracle, flags)))
        cum = [0]
        for off in range(0, cu8.size, BLOCK):
            blk = np.ascontiguousarray(cu8[off:off + BLOCK])
            L.wmo_feed(ctx, blk.ctypes.data, blk.size)
            cum.append(int(L.wmo_decimated_count(ctx)))
        L.wmo_free(ctx)
        pushes, a = [], 0
        first = {13: 11, 15: 8}[d]
        while a < len(cum) - 1:
            left = min(RAGGED_BLOCKS, len(cum) - 1 - a)
            cands = [nb for nb in range(1, left + 1) if (cum[a + nb] - cum[a]) % 64 == 4]
            nb = first if not pushes else (cands[0] if cands else min(left, -a % d or d))      # or the blocks that bring the phase back to 0
            pushes.append(nb); a += nb
        _ragged[d] = (cu8, flags, o, cum, pushes)
    return _ragged[d]


# ---- preconditions: no GPU ------------------------------------------------------------------------------------------------------
def test_the_run_cases_put_an_edge_of_either_kind_at_every_sample_of_a_word(oracle):
    for name in ("runs, noisy", "runs, clean"):
        _cu8, _o, ref = case(oracle, name)
        for ch in (0, 1):
            chip, reset = edge_ks(ref[ch].events)
            assert chip == set(range(64)) and reset == set(range(64)), (name, ch, sorted(set(range(64)) - chip), sorted(set(range(64)) - reset))
            ns = {e["n"] for e in ref[ch].events}
            assert ns >= set(range(1, 25)), (name, ch, sorted(set(range(1, 25)) - ns))


def test_noise_alone_is_the_reset_dense_regime(oracle):
    _cu8, _o, ref = case(oracle, "noise alone")
    for ch in (0, 1):
        kinds = [e["kind"] for e in ref[ch].events]
        resets = len(kinds) - kinds.count(rla_ref.CHIPS)
        assert resets > 1000 and 5 * resets > len(kinds), (ch, resets, len(kinds))      # a reset every hundred samples or so, at least every fifth edge (a telegram has none)
        chip, reset = edge_ks(ref[ch].events)
        assert reset == set(range(64))


def test_the_silences_give_the_long_runs_they_were_tuned_for(oracle):
    _cu8, _o, ref = case(oracle, "silences, samples")
    runs = [e["run"] for e in ref[0].events if e["run"] > 60000]
    assert runs == list(WANT_RUNS), runs
    _cu8, _o, ref2 = case(oracle, "silences, chips")
    ua, ua2 = ([e["div"][0][0] for e in r[0].events if e["run"] > 60000] for r in (ref, ref2))
    assert min(ua) >= 1 << 24 > max(ua2)                                       # the first division's dividend beyond wm_udiv's bound, and below it
    ns = [e["n"] for e in ref2[0].events if e["run"] > 60000]
    assert ns == list(WANT_CHIPS), ns
    for r in (ref, ref2):
        assert len(r[0].marker_samples()) == 3                                  # the access code behind every silence is found
        assert len([e for e in r[1].events if e["run"] > 60000]) == 3           # S1 sees three long runs too


@pytest.mark.parametrize("d", [13, 15])
def test_the_ragged_schedules_end_four_samples_into_a_word(wm, oracle, d):
    cu8, flags, o, cum, pushes = ragged_case(wm, oracle, d)
    ends = [(cum[b] - cum[a]) % 64 for a, b in zip(np.cumsum([0] + pushes[:-1]), np.cumsum(pushes))]
    assert cum[pushes[0]] == {13: 1732, 15: 1092}[d]
    assert ends.count(4) >= {13: 9, 15: 12}[d] and ends[0] == 4, ends           # pushes that end 4 samples into a word (kend < 5) ...
    assert d == 13 or any(ends[i:i + 3] == [4, 4, 4] for i in range(len(ends)))  # ... three of them in a row where the phase allows it
    assert sum(pushes) * BLOCK == cu8.size and max(pushes) <= RAGGED_BLOCKS
    # what whole blocks can reach at all, at any decimation: of the residues 1..4 only 4
    reach = {length % 64 for dd in range(1, 17) for nb in range(1, 2 * dd + 1) for length in (2048 * nb // dd, -(-2048 * nb // dd))}
    assert reach & {1, 2, 3, 4} == {4}


# ---- the compiled kernel ---------------------------------------------------------------------------------------------------------
def stream_and_compare(rx, cu8, o, push_blocks, what, stream=0):
    """Push by push: the slicer bits read back are the oracle's; those bits and the RSSI tap through rla_ref (state carried)
    give what wmbus_read_chips gives.  push_blocks: 4096-byte blocks per push.  Returns the pushes' re-run counts."""
    state, m0, a, reruns = [None, None], 0, 0, []
    for nb in push_blocks:
        rx.push([cu8[a * BLOCK:(a + nb) * BLOCK]])
        tm = rx.timing()
        assert tm["warnings"] == 0, what
        reruns.append(tm["rla_reruns"])
        m1 = None
        for ch in (0, 1):
            bits = rx.read_tap("bits", ch, stream, (nb * BLOCK) // 2)
            m1 = m0 + len(bits)
            assert np.array_equal(bits, o["bit"][ch][m0:m1]), what + (f"push at block {a}", "bits", ch)
            rssi = rx.read_tap("rssi", ch, stream, len(bits))
            r = rla_ref.run(ch, bits, rssi=rssi, start=state[ch], origin=m0)
            state[ch] = r.final
            want = r.chips(rssi=True)
            w, pos = rx.read_chips(ch, 0, stream, cap=1 << 20)
            at = what + (f"push at block {a}", f"samples {m0}..{m1}", f"chain {ch}")
            assert len(w) == len(want), at + (len(w), len(want))
            assert np.array_equal(pos, want[:, 0]), at + ("positions", np.flatnonzero(pos != want[:, 0])[:4])
            assert np.array_equal(w & 0xFF, want[:, 1]), at + ("values and markers", np.flatnonzero((w & 0xFF) != want[:, 1])[:4])
            assert np.array_equal((w >> 8) & 0xFF, want[:, 2]), at + ("RSSI bytes",)
        m0, a = m1, a + nb
    assert m0 == o["m"], what
    return reruns


@pytest.mark.gpu
@pytest.mark.parametrize("lookback", LOOKBACKS)
@pytest.mark.parametrize("name", list(CASES))
def test_designed_captures_chip_for_chip(wm, oracle, name, lookback):
    cu8, o, _ref = case(oracle, name)
    with wm.Receiver(n_streams=1, max_push_bytes=PUSH, rla_lookback=lookback, **SEGS) as rx:
        reruns = stream_and_compare(rx, cu8, o, [PUSH // BLOCK] * (cu8.size // PUSH), (name, f"look-back {lookback}"))
    assert sum(reruns) > 0 or rx.cfg.rounds_on_host, (name, lookback, reruns)     # at least one hand-off was not certified by the look-back


@pytest.mark.gpu
@pytest.mark.parametrize("lookback", LOOKBACKS)
@pytest.mark.parametrize("d", [13, 15])
def test_pushes_that_end_four_samples_into_a_word(wm, oracle, d, lookback):
    cu8, flags, o, _cum, pushes = ragged_case(wm, oracle, d)
    with wm.Receiver(n_streams=1, max_push_bytes=RAGGED_BLOCKS * BLOCK, rla_lookback=lookback, **SEGS, **flags_to_kwargs(flags)) as rx:
        stream_and_compare(rx, cu8, o, pushes, (f"-d {d}", f"look-back {lookback}"))


@pytest.mark.gpu
def test_the_run_case_as_two_contexts_in_one_lane(wm, oracle):
    """The noisy and the clean run capture as two contexts that share ONE lane, so that k2_rla_pair and k2_rla_list_pair see
    them: the chips of the last push of either context are the restatement's (on the oracle's bits, which the test above holds
    the GPU's to), in the lane run and in the lane-per-context run."""
    names = ("runs, noisy", "runs, clean")
    caps = [case(oracle, n)[0] for n in names]
    assert caps[0].size == caps[1].size
    n_push = caps[0].size // PUSH
    want = []
    for n in names:
        _cu8, o, ref = case(oracle, n)
        m0 = (n_push - 1) * PUSH // 4
        want.append([c[c[:, 0] >= m0] for c in (ref[ch].chips(rssi=True) for ch in (0, 1))])
        assert all(len(c) > 100 for c in want[-1])
    seen = []

    def after(b):
        seen.append([[rx.read_chips(ch, 0, 0, cap=1 << 20) for ch in (0, 1)] for rx, _first, _n in b.contexts])
    got = one_lane(wm, caps, 2, push=PUSH, n_push=n_push, input_windows=2, rla_lookback=32, after=after, **SEGS)
    assert got.plan == [(0, 1), (1, 1)] and len(seen) == 2
    assert any(tm["rla_reruns"] > 0 for tms in got.timing.values() for tm in tms)
    for run in seen:
        for s in (0, 1):
            for ch in (0, 1):
                w, pos = run[s][ch]
                c = want[s][ch]
                assert len(w) == len(c) and np.array_equal(pos, c[:, 0]) and np.array_equal(w & 0xFF, c[:, 1]) and np.array_equal((w >> 8) & 0xFF, c[:, 2]), (s, ch)


@pytest.mark.gpu
def test_the_kernels_integer_divisions_over_their_domain(wm):
    """wm_udiv / wm_sdiv (the functions the run-length kernel inlines) on the device against the compiler's division: every
    divisor 4..4095 with every multiple below 2^24 and its two neighbours, every divisor 1..8192 with the dividends around
    2^24 and 0..128, either sign.  No capture takes the kernel to these corners; tests/sdiv_check.cpp checks a copy of the
    formula on the host."""
    wrong, first, cases = wm.selftest_udiv()
    assert cases > 3.4e8, cases
    assert wrong == 0, (wrong, first)
