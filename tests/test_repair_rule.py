"""CRC repair (cfg.crc_repair): the rule of include/wmbus_hip.h, CRC REPAIR, as tests/repair_ref.py restates it, on the oracle's taps and
chips of the three captures the header names; and the ABI of the feature.  No GPU needed.

The bundled 1.6 MS/s capture: its second telegram fails the CRC of its last block in the time2 framer's copy (one invalid 3-out-of-6
symbol); the restatement repairs it by one chip.  Two synthetic captures near the discriminator's threshold: every repaired telegram
must equal the bytes that were sent.  The expected text and the counts are tests/golden/repair.json (python tests/repair_ref.py)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import repair_ref as RR
import telegram_ref as TR
from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with open(RR.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def bundled(oracle, samples):
    cu8 = samples["samples2"][:samples["samples2"].size // 4096 * 4096]
    ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
    return ref, RR.repair_capture(ref)


def test_bundled_capture_one_chip_repairs_the_second_telegram(bundled, golden):
    ref, res = bundled
    before = ref["text"].splitlines(keepends=True)
    assert len(before) == len(res["lines"]) == 4
    changed = [i for i in range(4) if res["lines"][i] != before[i]]
    assert changed == [2] and before[2].startswith("t2a;T1;0;0;") and before[2].rstrip().endswith("7cfaff6857c98d")
    assert res["subjects"] == 1 and res["repaired"] == [False, False, True, False]
    rec = res["records"][2]
    assert (rec["blocks_bad"], rec["blocks_repaired"], rec["chips_flipped"]) == (1, 1, 1) and 0 < rec["weight"] < 1 << 29
    assert [r for i, r in enumerate(res["records"]) if i != 2] == [RR.ZERO] * 3
    air = res["air"][2]
    assert len(air) == 117 and air[0] == 102 and air[-15:].hex() == "0b9c5f3adc3f7cfa326857c98da060"
    assert TR.crc_clean(False, air, len(air))
    assert res["lines"][2].startswith("t2a;T1;1;1;") and res["crc_ok"] == [1, 1, 1, 0]
    # the run-length framer's copy of that telegram is bad too, and stays: its chips carry no decision instant
    assert before[3].startswith("rla;T1;0;0;") and res["lines"][3] == before[3]
    g = golden["samples2"]
    assert (res["lines"], res["crc_ok"], res["records"], res["subjects"]) == (g["lines"], g["crc_ok"], g["records"], g["subjects"])


def test_bundled_capture_cut_into_pushes(bundled):
    """The cut is a parameter of the restatement: the telegram's chips lie in decimated samples 199 000 ... 208 400, so pushes of 2^16
    keep it whole and pushes of 2^12 cut it -- then it is no subject and nothing changes."""
    ref, res = bundled
    assert RR.repair_capture(ref, push_m=1 << 16)["lines"] == res["lines"]
    cut = RR.repair_capture(ref, push_m=1 << 12)
    assert cut["subjects"] == 0 and "".join(cut["lines"]) == ref["text"] and cut["records"] == [RR.ZERO] * 4


@pytest.mark.parametrize("name", list(RR.SYNTHETIC))
def test_synthetic_captures_repair_only_into_what_was_sent(oracle, golden, name):
    mode, sigma = RR.SYNTHETIC[name]
    cu8, sent = RR.synthetic(mode, sigma)
    ref = oracle.run(cu8, oracle.make_opts(), taps=True, chips=True)
    res = RR.repair_capture(ref)
    n = RR.counts(res, sent)
    print(name, n, "subjects", res["subjects"])
    assert n["false_repairs"] == 0 and n["repaired"] >= 1
    for air, rep in zip(res["air"], res["repaired"]):
        if rep:
            assert bytes(air) in sent
    assert n == golden["synthetic"][name]
    # a repaired line is a clean line: the verdict, the payload of the sent telegram
    for line, air, rep, ok in zip(res["lines"], res["air"], res["repaired"], res["crc_ok"]):
        if rep:
            assert ok == 1 and line.split(";")[2] == "1" and line.rstrip().endswith("0x" + TR.printed_hex(False, air, len(air)))


def test_the_restatement_by_hand():
    """One C1 block, chip for chip: the least reliable wrong chip is found, ties go to the lower chip, a pattern has to pass the CRC."""
    air = TR.frame_a(bytes([9]) + bytes(range(1, 10)))                       # one block of 12 bytes
    v = np.array(TR.chips("C1A", air), np.int64) & 1
    r = np.full(v.size, 1000, np.int64)
    bad = v.copy(); bad[17 + 8 * 3 + 2] ^= 1
    r[17 + 8 * 3 + 2] = 7
    res = RR.repair_telegram("C1", False, 12, bad, r)
    assert res["repaired"] and res["air"] == air and res["record"] == dict(blocks_bad=1, blocks_repaired=1, chips_flipped=1, weight=7)
    res = RR.repair_telegram("C1", False, 12, bad, np.full(v.size, 5, np.int64))        # all equal: the first eight chips behind the L-field
    assert not res["repaired"] and res["record"]["blocks_bad"] == 1
    bad = v.copy(); bad[17 + 8 + 7] ^= 1
    res = RR.repair_telegram("C1", False, 12, bad, np.full(v.size, 5, np.int64))
    assert res["repaired"] and res["record"]["weight"] == 5
    bad = v.copy(); bad[17 + 3] ^= 1                                          # in the L-field's byte: never a candidate
    r = np.full(v.size, 1000, np.int64); r[17 + 3] = 0
    assert not RR.repair_telegram("C1", False, 12, bad, r)["repaired"]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_abi_has_the_repair(wm):
    """Fails on a tree without the feature.  The field sits directly in front of rounds_on_host, from where on earlier features pin
    every field to its neighbours; nothing behind it moves."""
    names = [f[0] for f in wm.Cfg._fields_]
    i = names.index("crc_repair")
    assert names[i - 1] == "tolerance_mode" and names[i + 1:i + 3] == ["rounds_on_host", "channel_activity"]
    with open(os.path.join(ROOT, "include", "wmbus_hip.h")) as f:
        assert "directly in front of rounds_on_host" in f.read()
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(wmbus_cfg), '
                           'offsetof(wmbus_cfg, crc_repair), offsetof(wmbus_cfg, rounds_on_host), sizeof(wmbus_repair), offsetof(wmbus_repair, chips_flipped), '
                           'offsetof(wmbus_repair, weight));return 0;}\n')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split()))
    assert got == [ctypes.sizeof(wm.Cfg), wm.Cfg.crc_repair.offset, wm.Cfg.rounds_on_host.offset, ctypes.sizeof(wm.Repair), wm.Repair.chips_flipped.offset,
                   wm.Repair.weight.offset]
    assert ctypes.sizeof(wm.Repair) == 12 and wm.Cfg.rounds_on_host.offset == wm.Cfg.crc_repair.offset + 4
    c = wm.Cfg()
    c.crc_repair = 7
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.crc_repair == 0
    for name in ("wmbus_line_repairs", "wmbus_batch_line_repairs"):
        assert name in wm.EXPORTS and hasattr(wm.lib(), name)
    assert hasattr(wm.Receiver, "line_repairs")
    # without a context, and without a batch, the accessors return 0 / NULL
    p = ctypes.POINTER(wm.Repair)()
    assert wm.lib().wmbus_line_repairs(None, ctypes.byref(p)) == 0 and not p
    assert wm.lib().wmbus_batch_line_repairs(None, 0, ctypes.byref(p)) == 0 and not p


def test_the_field_is_validated_before_a_device_is_asked_for(wm):
    """WMBUS_EINVAL (-1) with a message, on any machine: above 1; together with bursts_to_host."""
    with pytest.raises(wm.WmbusError, match=r"\(-1\): crc_repair must be 0 or 1, got 2"):
        wm.Receiver(n_streams=1, crc_repair=2)
    with pytest.raises(wm.WmbusError, match=r"\(-1\): crc_repair .* bursts_to_host .* nothing it could repair"):
        wm.Receiver(n_streams=1, crc_repair=1, bursts_to_host=True)
    with pytest.raises(wm.WmbusError, match=r"crc_repair must be 0 or 1"):
        wm.Batch(n_streams=64, crc_repair=3)


def test_cli_knows_the_switch(wm):
    p = subprocess.run([wm.CLI_PATH, "-h"], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert p.stdout.count("\t-x repair time2 telegrams that fail a block CRC") == 1
