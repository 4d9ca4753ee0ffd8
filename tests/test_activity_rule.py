"""Channel activity (cfg.channel_activity), the host side: the ABI; wmbus_activity_rule and wmbus_activity_match through ctypes against
the restatement tests/activity_ref.py on constructed timelines -- every edge of the rule.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import activity_ref as AR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = AR.cases()


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    """Everything here describes cfg.channel_activity: on a library without the field no test of this file says anything, so none passes."""
    assert "channel_activity" in [f[0] for f in wm.Cfg._fields_] and "wmbus_activity_rule" in wm.EXPORTS


def test_the_abi_has_the_activity_fields(wm, tmp_path):
    """The two fields lie next to each other in front of rssi_full; nothing behind them moves relative to the end of the struct;
    wmbus_timing keeps its 152 bytes, wmbus_burst is 32 bytes; header and mirror agree on every size and offset."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("channel_activity")
    assert names[k - 1:k + 5] == ["rounds_on_host", "channel_activity", "channel_activity_ratio_q8", "rssi_full", "rssi_dense_pm", "line_power"]
    c = wm.Cfg()
    c.channel_activity = c.channel_activity_ratio_q8 = 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.channel_activity == 0 and c.channel_activity_ratio_q8 == 0
    assert wm._make_cfg(channel_activity=1, channel_activity_ratio_q8=512).channel_activity_ratio_q8 == 512 and wm._make_cfg().channel_activity == 0
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned channel_activity;", "unsigned channel_activity_ratio_q8;", "CHANNEL ACTIVITY (cfg.channel_activity = 1",
                 "size_t wmbus_activity(const wmbus_ctx *ctx, const wmbus_burst **records);",
                 "long wmbus_activity_rule(const uint32_t *p, size_t n, unsigned in_hz, unsigned ratio_q8, wmbus_burst *out, size_t cap);",
                 "long wmbus_activity_match(const wmbus_burst *records, size_t n, unsigned stream, unsigned channel, int chain, uint64_t ka);",
                 "size_t wmbus_batch_activity(const wmbus_batch *b, unsigned first_stream, const wmbus_burst **records);",
                 "H = min(63, ceil(0.16 Fin / 32768) + 1)", "act[K] = (P[K] x 256 > T x floor[e(K)])", "first_block - 1 <= ka < first_block + blocks",
                 "(748, 21) and (1424, 46)", "rests on these two captures and on synthetic noise only"):
        assert word in hdr, word
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, channel_activity), offsetof(wmbus_cfg, channel_activity_ratio_q8), offsetof(wmbus_cfg, rssi_full), offsetof(wmbus_cfg, line_power), '
                   'sizeof(wmbus_burst), offsetof(wmbus_burst, stream), offsetof(wmbus_burst, chain), sizeof(wmbus_cfg));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()))
    assert got == [152, wm.Cfg.channel_activity.offset, wm.Cfg.channel_activity_ratio_q8.offset, wm.Cfg.rssi_full.offset, wm.Cfg.line_power.offset,
                   ctypes.sizeof(wm.Burst), wm.Burst.stream.offset, wm.Burst.chain.offset, ctypes.sizeof(wm.Cfg)]
    assert ctypes.sizeof(wm.Burst) == 32 and wm.Cfg.rssi_full.offset == wm.Cfg.channel_activity.offset + 8
    assert hasattr(wm.Receiver, "activity")


def test_the_cases_hold_what_they_are_named_for():
    """The constructed timelines reach the edges they claim: checked on the restatement, so a change to a case shows here."""
    fin = 1600000
    H = AR.epochs_back(fin)
    assert H == 9 and AR.epochs_back(12800000) == 63 and AR.epochs_back(800000) == 5 and AR.epochs_back(12595200) == 63 and AR.epochs_back(12492800) == 62
    r = {k: AR.rule(*v) for k, v in CASES.items()}
    assert r["all_equal"] == []
    assert [(b["first_block"], b["blocks"], b["floor"]) for b in r["floor_zero"]] == [(5, 3, 0), (64, 2, 0)]
    assert [(b["first_block"], b["blocks"]) for b in r["len_1_and_2"]] == [(20, 2), (100, 2)]
    assert [(b["first_block"], b["blocks"]) for b in r["lane_0_and_63"]] == [(64, 5), (120, 8), (190, 2)]      # (254, 2) ends the stream: never closed
    assert [(b["first_block"], b["blocks"]) for b in r["two_epochs"]] == [(60, 10), (127, 2)]
    assert [(b["first_block"], b["blocks"]) for b in r["three_epochs"]] == [(50, 100)]
    assert [(b["first_block"], b["blocks"]) for b in r["whole_epoch_inside"]] == [(100, 158)]
    ff = r["floor_forgets"]                                  # while the quiet epoch is remembered 1800 is active (runs of one: dropped) and 5000 joins nothing new
    assert ff[0]["first_block"] == 70 and ff[0]["floor"] == 400 and ff[-1]["first_block"] == 64 * (H + 3) + 9 and ff[-1]["floor"] >= 1000
    car = r["carrier"]
    assert len(car) == 1 and car[0]["first_block"] == 100 and car[0]["blocks"] == 64 * (H + 2) - 100      # epochs 1 ... H + 1 hold it wholly: closed at the start of epoch H + 2
    hc = r["h_clamp"]
    assert (hc[0]["first_block"], hc[0]["blocks"]) == (67, 64 * 64 - 67)                                  # H = 63: epoch 64's floor no longer sees epoch 0 (an unclamped H = 64 would)
    assert [(b["first_block"], b["blocks"]) for b in hc[1:]] == [(64 * 67, 3)]                            # its last three blocks share an epoch with silence: the floor is back
    assert [(b["first_block"], b["blocks"]) for b in r["T_257"]] == [(10, 2), (40, 2)]
    assert [(b["first_block"], b["blocks"]) for b in r["T_1024"]] == [] and r["T_65535"] == []
    assert [(b["first_block"], b["blocks"]) for b in r["T_65535_hits"]] == [(80, 2)]
    assert [(b["first_block"], b["blocks"]) for b in r["trailing"]] == [(30, 6)]
    assert len(r["random"]) >= 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_rule_is_the_restatement(wm, name):
    p, fin, T = CASES[name]
    want = AR.rule(p, fin, T)
    got = wm.activity_rule(p, fin, T)
    assert AR.strip(got) == want
    assert all(b["stream"] == 0 and b["channel"] == 0 and b["chain"] == 0 for b in got)
    if T == 0:
        assert AR.strip(wm.activity_rule(p, fin, 1024)) == want           # 0 means 1024


def test_the_rule_at_other_thresholds_and_rates(wm):
    p = CASES["random"][0]
    for fin in (800000, 1600000, 2400000, 4000000, 12800000):
        for T in (257, 300, 512, 1024, 2048, 65535):
            assert AR.strip(wm.activity_rule(p, fin, T)) == AR.rule(p, fin, T), (fin, T)


def test_the_rule_refuses_what_the_field_refuses(wm):
    L = wm.lib()
    p = np.arange(128, dtype=np.uint32)
    out = (wm.Burst * 8)()
    for bad in (1, 256, 65536, 1 << 20):
        assert L.wmbus_activity_rule(p.ctypes.data, p.size, 1600000, bad, out, 8) == -1
    assert L.wmbus_activity_rule(p.ctypes.data, p.size, 799999, 0, out, 8) == -1
    assert L.wmbus_activity_rule(None, 5, 1600000, 0, out, 8) == -1
    assert L.wmbus_activity_rule(p.ctypes.data, p.size, 1600000, 0, None, 8) == -1
    assert L.wmbus_activity_rule(None, 0, 1600000, 0, None, 0) == 0
    # more found than cap: the count is the number found, only cap are written
    q, fin, T = CASES["lane_0_and_63"]
    small = (wm.Burst * 2)()
    assert L.wmbus_activity_rule(q.ctypes.data, q.size, fin, T, small, 2) == 3 and small[1].first_block == 120


def test_matching_on_every_edge(wm):
    """first_block - 1 <= ka < first_block + blocks, on the row of the line only."""
    rec = [dict(first_block=0, blocks=3, mean=1, floor=1, stream=0, channel=0, chain=0),
           dict(first_block=20, blocks=5, mean=1, floor=1, stream=0, channel=0, chain=0),
           dict(first_block=26, blocks=2, mean=1, floor=1, stream=0, channel=0, chain=0),
           dict(first_block=20, blocks=5, mean=1, floor=1, stream=1, channel=2, chain=1)]
    row0 = rec[:3]
    for ka, want in ((0, 0), (2, 0), (3, -1), (18, -1), (19, 1), (20, 1), (24, 1), (25, 2), (26, 2), (27, 2), (28, -1), (1 << 40, -1)):
        assert AR.match(row0, ka) == want, ka
        assert wm.activity_match(rec, 0, 0, 0, ka) == want, ka
    assert wm.activity_match(rec, 1, 2, 1, 19) == 3 and wm.activity_match(rec, 1, 2, 1, 24) == 3 and wm.activity_match(rec, 1, 2, 1, 25) == -1
    for row in ((1, 2, 0), (1, 0, 1), (0, 2, 1), (2, 0, 0)):
        assert wm.activity_match(rec, *row, 22) == -1
    assert wm.activity_match([], 0, 0, 0, 5) == -1
