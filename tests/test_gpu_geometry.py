"""Push geometry at every decimation on the compiled kernels: pushes whose segments end at the smallest and the largest
residue a whole number of 4096-byte blocks can reach, at decimations the other GPU suites never stream (the run-time-D
demodulation path, its decimation phase carried across pushes), with exact silence after a signal.  Push by push, the soft
symbols, RSSI, slicer bits and the chips of both framers are compared with the oracle's slice of that push, bit for bit, in
both clock-recovery forms, for one capture and for a batch of 64 (the cooperative loads), after short and long warm-ups."""
import ctypes

import numpy as np
import pytest

from cases import flags_to_kwargs, flags_to_oracle_opts
from test_gpu_fuzz import truncate_runs

pytestmark = pytest.mark.gpu

BLOCK = 4096                                                  # bytes: the unit of a push (wmbus_process)
DECIMATIONS = [3, 5, 6, 7, 9, 11, 12, 13, 14, 15]
WARM = {"short": dict(warmup_t1c1=512, warmup_s1=512), "long": dict(warmup_t1c1=12288, warmup_s1=24576)}
FORMS = {1: "one-wave", 4: "systolic"}
_captures = {}


def capture(wm, oracle, d, seg_len):
    """Signal, exact silence (127), signal, exact silence (128) (3 : 1 : 3 : 1); the oracle's taps and chips over all of it, and the
    oracle's decimated count after every block (a push of blocks a .. b is cum[b] - cum[a] samples long)."""
    key = (d, seg_len)
    if key not in _captures:
        m_total = max(65536, 16 * seg_len)
        cu8 = wm.synth_capture(seed=5150 + d, n_samples=m_total * d, fs_khz=800 * d, kinds=15, frames_per_s=400.0, amplitude=60.0)[0]
        cu8 = cu8[: cu8.size // BLOCK * BLOCK]
        e = cu8.size // 8 // 2 * 2
        cu8[3 * e:4 * e] = 127
        cu8[7 * e:] = 128
        flags = ["-v", "-d", str(d)]
        ref = oracle.run(cu8, flags_to_oracle_opts(oracle, flags), taps=True, chips=True)
        L = oracle.lib()
        ctx = L.wmo_new(ctypes.byref(flags_to_oracle_opts(oracle, flags)))
        cum = [0]
        for off in range(0, cu8.size, BLOCK):
            blk = np.ascontiguousarray(cu8[off:off + BLOCK])
            L.wmo_feed(ctx, blk.ctypes.data, blk.size)
            cum.append(int(L.wmo_decimated_count(ctx)))
        L.wmo_free(ctx)
        assert cum[-1] == ref["m"]
        _captures[key] = (cu8, flags, ref, cum)
    return _captures[key]


def schedule(cum, seg_len, max_blocks):
    """Block counts of the pushes: in turn the one whose last segment ends at the smallest nonzero residue, then the largest,
    among pushes of up to max_blocks blocks (holding a whole segment where one can)."""
    pushes, a, n, k = [], 0, len(cum) - 1, 0
    while a < n:
        cands = [(b - a, (cum[b] - cum[a]) % seg_len, cum[b] - cum[a]) for b in range(a + 1, min(n, a + max_blocks) + 1)]
        good = [c for c in cands if c[1] and c[2] >= seg_len] or [c for c in cands if c[1]] or cands
        pick = min(good, key=lambda c: c[1]) if k % 2 == 0 else max(good, key=lambda c: c[1])
        pushes.append(pick[0])
        a += pick[0]
        k += 1
    return pushes


def oracle_chips(ref, ch, al, m0, m1):
    oc = ref["chips"][(ref["chips"]["chain"] == ch) & (ref["chips"]["algo"] == al) & (ref["chips"]["sample"] >= m0) & (ref["chips"]["sample"] < m1)]
    return truncate_runs(oc)


@pytest.mark.parametrize("seg_len", [1024, 4096])
@pytest.mark.parametrize("d", DECIMATIONS)
def test_push_geometry_at_every_decimation(wm, oracle, d, seg_len):
    cu8, flags, ref, cum = capture(wm, oracle, d, seg_len)
    max_blocks = min(64, -(-3 * seg_len * d * 2 // BLOCK))     # pushes up to three segments long
    pushes = schedule(cum, seg_len, max_blocks)
    residues = [(cum[b] - cum[a]) % seg_len for a, b in zip(np.cumsum([0] + pushes[:-1]), np.cumsum(pushes))]
    assert len(set(residues) - {0}) >= 2, residues
    kw = flags_to_kwargs(flags)
    for S in (1, 64):
        for warm in ("short", "long"):
            rounds0 = {}
            for waves, form in FORMS.items():
                what = (form, f"S={S}", f"warm={warm}")
                with wm.Receiver(n_streams=S, max_push_bytes=max_blocks * BLOCK, seg_len=seg_len, rla_seg_len=seg_len, clock_waves=waves,
                                 **WARM[warm], **kw) as rx:
                    text, a, s = "", 0, S - 1
                    rounds0[waves] = []
                    for nb in pushes:
                        m0, m1 = cum[a], cum[a + nb]
                        blk = cu8[a * BLOCK:(a + nb) * BLOCK]
                        rx.push([blk] * S)
                        text += "".join(ln["text"] for ln in rx.lines() if ln["stream"] == s)
                        rounds0[waves].append(rx.timing()["clock_round"][0])
                        at = what + (f"push at block {a}", f"{m1 - m0} samples")
                        for ch in (0, 1):
                            dphi = rx.read_tap("dphi", ch, s, m1 - m0 + 1)
                            assert len(dphi) == m1 - m0, at
                            assert np.array_equal(dphi.view(np.uint32), ref["dphi_fir"][ch][m0:m1].view(np.uint32)), at + ("dphi", ch)
                            rssi = rx.read_tap("rssi", ch, s, m1 - m0)
                            assert np.array_equal(rssi, ref["rssi"][ch][m0:m1].astype(np.uint32).astype(np.uint8)), at + ("rssi", ch)
                            bits = rx.read_tap("bits", ch, s, m1 - m0)
                            assert np.array_equal(bits, ref["bit"][ch][m0:m1]), at + ("bits", ch, np.flatnonzero(bits != ref["bit"][ch][m0:m1])[:8])
                            for al in (0, 1):
                                w, pos = rx.read_chips(ch, al, s, cap=1 << 18)
                                oc = oracle_chips(ref, ch, al, m0, m1)
                                assert len(w) == len(oc), at + ("chips", ch, al, len(w), len(oc))
                                assert (np.array_equal(w & 0xFF, oc["value"]) and np.array_equal((w >> 8) & 0xFF, oc["rssi"])
                                        and np.array_equal(pos, oc["sample"])), at + ("chips", ch, al)
                        a += nb
                    assert text == ref["text"], what
            # the first pass is deterministic and the same in both forms: so are the segments it leaves uncertified (none are counted
            # where the host finishes the hand-offs, WMBUS_TEST_ROUNDS_ON_HOST)
            assert rounds0[1] == rounds0[4], ("round-0 re-runs by push", f"S={S}", f"warm={warm}", rounds0)
            assert warm == "long" or rx.cfg.rounds_on_host or sum(rounds0[4]) > 0, ("no re-run after short warm-ups", f"S={S}", rounds0)
