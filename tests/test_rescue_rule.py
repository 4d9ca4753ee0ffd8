"""S1 rescue (cfg.s1_rescue): the rule of include/wmbus_hip.h, S1 RESCUE, as tests/rescue_ref.py restates it, on the oracle's taps and
chips of two synthetic S1 captures near the discriminator's threshold and of a clean one; and the ABI of the feature.  No GPU needed.

The counts of the two captures are tests/golden/rescue.json (python tests/rescue_ref.py): every rescued telegram must equal the bytes
that were sent.  The bundled captures hold no S1 telegram that aborts at a Manchester pair: the rule has no subject there."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import level_ref as LR
import rescue_ref as RF
import telegram_ref as TR
from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with open(RF.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(oracle):
    """name -> (ref, restatement, sent) of the two synthetic captures: computed once, shared, left unchanged."""
    out = {}
    for name in RF.SYNTHETIC:
        cu8, sent = RF.synthetic(name)
        ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
        out[name] = (ref, RF.rescue_capture(ref), sent)
    return out


@pytest.mark.parametrize("name", list(RF.SYNTHETIC))
def test_synthetic_captures_rescue_only_what_was_sent(runs, golden, name):
    ref, res, sent = runs[name]
    n = RF.counts(res, sent)
    print(name, n)
    # a capture that rescues nothing cannot pass: rescues, something the gate (or a CRC) leaves out, something the oracle decodes anyway
    assert n["rescued"] >= 3 and (n["gated"] >= 1 or n["bad"] >= 1) and n["decoded"] >= 1
    assert n["false_rescues"] == 0 and n == golden[name]
    plain = ref["text"].splitlines(keepends=True)
    for line, air, rescued, ok, rec, k in zip(res["lines"], res["air"], res["rescued"], res["crc_ok"], res["records"], res["plain"]):
        if rescued:
            assert bytes(air) in sent and ok == 1 and k is None and rec["status"] == 1 and rec["pairs"] >= 1 and rec["blocks"] == RF.n_blocks(len(air))
            assert line.startswith("t2a;S1;1;1;TS;") and line.rstrip().endswith("0x" + TR.printed_hex(False, air, len(air)))
            assert line not in plain                            # the oracle prints nothing for it: that is the loss
        else:
            assert rec == RF.ZERO and line == plain[k]
    assert [k for k in res["plain"] if k is not None] == list(range(len(plain)))      # every other line, in the oracle's order


def test_the_mixed_capture_covers_the_lengths(runs):
    """L-field 255 (290 bytes, 17 blocks, 4641 chips) among the rescued of the mixed capture, beside a shorter one."""
    _, res, _ = runs["s1-mixed"]
    blocks = sorted(rec["blocks"] for rec in res["records"] if rec["status"] == 1)
    assert blocks[-1] == 17 and blocks[0] <= 3


def test_the_cut_is_a_parameter(runs):
    """Pushes of 2^15 decimated samples: a telegram of L-field 40 is 18 400 samples long, so some straddle an edge and are no subjects."""
    ref, res, _ = runs["s1-l40"]
    cut = RF.rescue_capture(ref, push_m=1 << 15)
    assert 0 < cut["stats"][1] < res["stats"][1] and cut["stats"][0] == cut["stats"][1] + len(cut["bad"])
    assert RF.rescue_capture(ref, push_m=1 << 12)["stats"] == (0, 0)


def test_the_bundled_captures_hold_no_subject(oracle, samples):
    for name, opts in (("samples2", {}), ("issue48", dict(decimation=3, simultaneous=1))):
        cu8 = samples[name][:samples[name].size // 4096 * 4096]
        ref = oracle.run(cu8, oracle.make_opts(**opts), taps=True, chips=True)
        res = RF.rescue_capture(ref)
        assert res["stats"] == (0, 0) and res["gated"] == 0 and "".join(res["lines"]) == ref["text"], name


def test_polarity_on_a_clean_telegram(oracle):
    """"1 is the larger soft symbol": on a clean S1 telegram every pair is valid, and in every pair the chip that reads 1 has the larger
    quantised soft symbol -- the decision the rule makes for an invalid pair is the one the slicer makes for a valid one."""
    air = TR.frame_a(bytes([40]) + bytes(np.random.default_rng(7).integers(0, 256, 40).astype(np.uint8)))
    cu8 = TR.modulate([("S1", air)], seed=1, amplitude=60, sigma=2.0)
    ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
    events, val, rssi, pos = RF.walk(ref, 1, 1)
    done = [e for e in events if e["done"]]
    assert len(done) == 1 and done[0]["bytes"] == air and done[0]["crc_ok"]
    i, n = done[0]["i"], done[0]["consumed"]
    v = val[i + 1:i + n] & 1
    q = LR.quantise(np.asarray(ref["dphi_fir"][1], np.float32)[pos[i + 1:i + n]])
    a, b = v[0::2], v[1::2]
    assert (a != b).all() and len(a) == 8 * len(air)
    assert ((q[1::2] > q[0::2]) == (b == 1)).all()
    bits, pairs, margin = RF.decide(v, q)
    assert pairs == 0 and margin is None and bits == [int(x) for x in b]
    # and with every pair made invalid the soft decision alone gives the telegram back
    res = RF.rescue_telegram(len(air), np.zeros_like(v), q)
    assert res["rescued"] and res["air"] == air and res["record"]["pairs"] == 8 * len(air) and res["record"]["min_margin"] > 0


def chips_of(air, wrong=()):
    v = np.array(TR.chips("S1", air), np.int64)
    for j in wrong:
        v[j] ^= 1
    return v


def test_the_decision_by_hand():
    """Valid pairs keep their value whatever the soft symbols say; an invalid pair goes to the larger soft symbol; a tie reads 0."""
    v = [0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0]
    q = [9, -9, -9, 9, 5, 7, -3, -8, 4, 4, -6, -6]
    assert RF.decide(v, q) == ([1, 0, 1, 0, 0, 0], 4, 0)
    assert RF.decide(v[:8], q[:8]) == ([1, 0, 1, 0], 2, 2)


def test_subjects_by_hand():
    air = TR.frame_a(bytes([40]) + bytes(range(40)))
    L = len(air)
    n = 1 + 16 * L
    j = 1 + 2 * 100                                          # the first chip of data pair 100
    rssi = np.full(n + 32, 40, np.int64)
    v = chips_of(air, [j])
    assert RF.examine(v, rssi, 2 * 100 + 3) == ("subject", L)
    # consumed not at the first invalid pair: an RSSI abort in front of it, or the decoder went on -- no subject
    assert RF.examine(v, rssi, 150) == ("no", L) and RF.examine(v, rssi, 2 * 100 + 5) == ("no", L)
    e = TR.expect("S1", v, np.where(np.arange(n + 32) == 149, 4, 40))
    assert not e["done"] and e["consumed"] == 150
    assert TR.expect("S1", v, rssi)["consumed"] == 2 * 100 + 3
    # a second invalid pair behind the first changes nothing about the subject
    assert RF.examine(chips_of(air, [j, j + 50]), rssi, 2 * 100 + 3) == ("subject", L)
    # the gate: chip n - 2 counts, chip n - 1 (the completing chip) is exempt, as is the access-code chip; 5 passes
    for at, level, kind in ((n - 2, 4, "gated"), (n - 1, 4, "subject"), (n - 1, 0, "subject"), (0, 0, "subject"), (n - 2, 5, "subject"), (1, 4, "gated")):
        r = rssi.copy(); r[at] = level
        assert RF.examine(v, r, 2 * 100 + 3) == (kind, L), (at, level)
    # a framer reset on any chip 1 ... n - 1
    for at in (j + 9, n - 1):
        w = v.copy(); w[at] |= 4
        assert RF.examine(w, rssi, 2 * 100 + 3) == ("gated", L)
    # L < 12: L-field 8 is 11 air bytes; L-field 9 is 12, the smallest subject
    for lf, kind in ((8, "no"), (9, "subject")):
        short = TR.frame_a(bytes([lf]) + bytes(lf))
        assert len(short) == lf + 3
        assert RF.examine(chips_of(short, [1 + 2 * 20]), rssi, 2 * 20 + 3) == (kind, len(short))
    # an invalid pair inside the L-field: the length is unknown, an abort as today
    assert RF.examine(chips_of(air, [1 + 2 * 3]), rssi, 2 * 3 + 3) == ("no", 0)
    # the stream ends before chip n - 1
    assert RF.examine(v[:n - 1], rssi, 2 * 100 + 3) == ("short", L)


def test_verdict_by_hand():
    """All or nothing over the block CRCs: a decision that gives a wrong bit leaves a bad block, status 2."""
    air = TR.frame_a(bytes([26]) + bytes(range(26)))         # 33 bytes: 12 + 18 + 3
    L = len(air)
    v = chips_of(air)[1:1 + 16 * L] & 1
    q = np.where(v == 1, 1000, -1000)
    k = 2 * (8 * 31 + 4)                                     # a pair of the last block
    bad = v.copy(); bad[k] ^= 1
    res = RF.rescue_telegram(L, bad, q)
    assert res["rescued"] and res["air"] == air and res["record"] == dict(status=1, pairs=1, min_margin=2000, blocks=3)
    q2 = q.copy(); q2[k], q2[k + 1] = q[k + 1], q[k]          # the soft symbols say the opposite
    res = RF.rescue_telegram(L, bad, q2)
    assert not res["rescued"] and res["air"] is None and res["record"] == dict(status=2, pairs=1, min_margin=2000, blocks=3)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_abi_has_the_rescue(wm):
    """Fails on a tree without the feature.  The field sits directly in front of input_windows, a seam no earlier feature pins; from
    line_quality on every field keeps its neighbours."""
    names = [f[0] for f in wm.Cfg._fields_]
    i = names.index("s1_rescue")
    assert names[i - 1] == "only_crc_ok" and names[i + 1:i + 3] == ["input_windows", "line_quality"]
    with open(os.path.join(ROOT, "include", "wmbus_hip.h")) as f:
        assert "directly in\n     * front of input_windows" in f.read()
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wmbus_cfg), '
                           'offsetof(wmbus_cfg, s1_rescue), offsetof(wmbus_cfg, input_windows), sizeof(wmbus_rescue), offsetof(wmbus_rescue, pairs), '
                           'offsetof(wmbus_rescue, min_margin), offsetof(wmbus_rescue, blocks), sizeof(wmbus_timing));return 0;}\n')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(wm.Cfg), wm.Cfg.s1_rescue.offset, wm.Cfg.input_windows.offset, ctypes.sizeof(wm.Rescue), wm.Rescue.pairs.offset,
                   wm.Rescue.min_margin.offset, wm.Rescue.blocks.offset, ctypes.sizeof(wm.Timing)]
    assert ctypes.sizeof(wm.Rescue) == 12 and wm.Cfg.input_windows.offset == wm.Cfg.s1_rescue.offset + 4 and ctypes.sizeof(wm.Timing) == 152
    c = wm.Cfg()
    c.s1_rescue = 7
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.s1_rescue == 0
    for name in ("wmbus_line_rescues", "wmbus_batch_line_rescues", "wmbus_rescue_stats"):
        assert name in wm.EXPORTS and hasattr(wm.lib(), name)
    assert hasattr(wm.Receiver, "line_rescues") and hasattr(wm.Receiver, "rescue_stats")
    # without a context, and without a batch, the accessors return 0 / NULL
    p = ctypes.POINTER(wm.Rescue)()
    assert wm.lib().wmbus_line_rescues(None, ctypes.byref(p)) == 0 and not p
    assert wm.lib().wmbus_batch_line_rescues(None, 0, ctypes.byref(p)) == 0 and not p
    s, r = ctypes.c_uint(5), ctypes.c_uint(5)
    assert wm.lib().wmbus_rescue_stats(None, ctypes.byref(s), ctypes.byref(r)) == -1 and (s.value, r.value) == (0, 0)


def test_the_field_is_validated_before_a_device_is_asked_for(wm):
    """WMBUS_EINVAL (-1) with a message, on any machine: above 1; with bursts_to_host; without the S1 chain; without the time2 framer."""
    with pytest.raises(wm.WmbusError, match=r"\(-1\): s1_rescue must be 0 or 1, got 2"):
        wm.Receiver(n_streams=1, s1_rescue=2)
    with pytest.raises(wm.WmbusError, match=r"\(-1\): s1_rescue .* bursts_to_host .* nothing it could rescue"):
        wm.Receiver(n_streams=1, s1_rescue=1, bursts_to_host=True)
    with pytest.raises(wm.WmbusError, match=r"\(-1\): s1_rescue .* s1_enabled = 0"):
        wm.Receiver(n_streams=1, s1_rescue=1, s1=False)
    with pytest.raises(wm.WmbusError, match=r"\(-1\): s1_rescue .* time2_enabled = 0"):
        wm.Receiver(n_streams=1, s1_rescue=1, time2=False)
    with pytest.raises(wm.WmbusError, match=r"s1_rescue must be 0 or 1"):
        wm.Batch(n_streams=64, s1_rescue=3)


def test_cli_knows_the_switch(wm):
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert p.stdout.count("\t-y rescue S1 telegrams of the time2 framer that are lost to a Manchester violation") == 1
