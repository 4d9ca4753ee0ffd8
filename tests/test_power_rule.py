"""Channel power (cfg.line_power), the host side: the ABI; wmbus_line_power_rule and wmbus_line_power_block through ctypes against the
restatement tests/power_ref.py, on random timelines and on every edge of the rule; the channel window the kernel and the host share
against the restatement.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import power_ref as PW
from test_power_emulated import load_emu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RATES = [800000, 1600000, 2400000, 4000000, 10000000]


@pytest.fixture(autouse=True)
def the_library_has_the_feature(wm):
    assert "line_power" in [f[0] for f in wm.Cfg._fields_] and "wmbus_line_power_rule" in wm.EXPORTS


def test_the_abi_has_the_power_field(wm, tmp_path):
    """Fails on a tree without the feature.  The field sits directly in front of bursts_to_host; nothing behind it moves relative to the
    end of the struct; wmbus_timing keeps its 152 bytes, wmbus_power is 24 bytes."""
    names = [f[0] for f in wm.Cfg._fields_]
    k = names.index("line_power")
    assert names[k - 1] == "rssi_dense_pm" and names[k + 1:k + 3] == ["bursts_to_host", "input_spectrum_age"]
    c = wm.Cfg()
    c.line_power = 99
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.line_power == 0 and wm._make_cfg(line_power=1).line_power == 1 and wm._make_cfg().line_power == 0
    hdr = open(os.path.join(ROOT, "include", "wmbus_hip.h")).read()
    for word in ("unsigned line_power;", "CHANNEL POWER (cfg.line_power = 1",
                 "typedef struct wmbus_power { uint64_t first_block; uint32_t signal, noise, ratio_q8; uint16_t n_signal, n_noise; } wmbus_power;",
                 "size_t wmbus_line_power(const wmbus_ctx *ctx, const wmbus_power **power);",
                 "long wmbus_read_waterfall(wmbus_ctx *ctx, unsigned capture, uint32_t *rows, uint64_t *first_block, size_t cap_rows);",
                 "long wmbus_read_channel_power(wmbus_ctx *ctx, int chain, unsigned stream_v, uint32_t *p, uint64_t *first_block, size_t cap);",
                 "size_t wmbus_batch_line_power(const wmbus_batch *b, unsigned first_stream, const wmbus_power **power);",
                 "cb = 256 + floor((1024 f_r + Fin) / (2 Fin))", "j0 = min(lo >> 4, 32 - nb)", "G = ceil(Fin / 51200)", "Nn = ceil(Fin / 25600)"):
        assert word in hdr, word
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wmbus_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(wmbus_timing), '
                   'offsetof(wmbus_cfg, line_power), offsetof(wmbus_cfg, bursts_to_host), sizeof(wmbus_power), sizeof(wmbus_cfg));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "s")], capture_output=True, text=True).stdout.split()))
    assert got == [152, wm.Cfg.line_power.offset, wm.Cfg.bursts_to_host.offset, ctypes.sizeof(wm.Power), ctypes.sizeof(wm.Cfg)]
    assert ctypes.sizeof(wm.Power) == 24 and wm.Cfg.bursts_to_host.offset == wm.Cfg.line_power.offset + 4
    assert all(hasattr(wm.Receiver, n) for n in ("line_power", "read_waterfall", "read_channel_power"))


def both(wm, p, first, ka, ke, fin):
    want = PW.line_record(p, first, ka, ke, fin)
    got = wm.line_power_rule(p, first, ka, ke, fin)
    assert got == want, (first, ka, ke, fin, got, want)
    return got


@pytest.mark.parametrize("fin", RATES)
def test_rule_in_c_equals_the_restatement_on_random_timelines(wm, fin):
    """Timelines of 3000 level blocks over the whole range of a uint32 (a quarter of them small, so that quartiles and floors matter),
    starting at block 0 and deep inside a stream; telegrams anywhere, also reaching outside the array."""
    rng = np.random.default_rng(fin)
    G, Nn = PW.guard(fin)
    for first in (0, 5, (1 << 40) + 17):
        p = rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)
        p[rng.random(p.size) < 0.25] >>= 20
        for _ in range(300):
            ka = first + int(rng.integers(-10 if first else 0, p.size + 10))
            ke = ka + int(rng.integers(0, 700))
            both(wm, p, first, max(ka, 0), max(ke, 0), fin)
    assert wm.lib().wmbus_line_power_rule(None, 0, 0, 1, 2, 799999, ctypes.byref(wm.Power())) == -1
    assert wm.lib().wmbus_line_power_rule(None, 0, 0, 1, 2, fin, None) == -1
    assert wm.line_power_rule(np.zeros(0, np.uint32), 0, 1, 2, fin) == dict(first_block=1, signal=0, noise=0, ratio_q8=0, n_signal=0, n_noise=0)


@pytest.mark.parametrize("fin", RATES)
def test_rule_edges(wm, fin):
    G, Nn = PW.guard(fin)
    assert (G, Nn) == ((fin + 51199) // 51200, (fin + 25599) // 25600)
    rng = np.random.default_rng(1 + fin)
    p = rng.integers(1000, 2000, 4 * (G + Nn) + 100, dtype=np.uint64).astype(np.uint32)
    # ka < G: no noise block -- and so no ratio
    r = both(wm, p, 0, G - 1, G + 20, fin)
    assert r["n_noise"] == 0 and r["ratio_q8"] == 0 and r["n_signal"] == 20 and r["noise"] == 0
    r = both(wm, p, 0, G, G + 20, fin)
    assert r["n_noise"] == 0
    r = both(wm, p, 0, G + 1, G + 20, fin)
    assert r["n_noise"] == 1 and r["noise"] == int(p[0])
    # ka - G - Nn < 0: a short noise window
    r = both(wm, p, 0, G + Nn - 3, G + Nn + 9, fin)
    assert r["n_noise"] == Nn - 3 and r["noise"] == sorted(int(v) for v in p[:Nn - 3])[(Nn - 3) // 4]
    r = both(wm, p, 0, G + Nn, G + Nn + 9, fin)
    assert r["n_noise"] == Nn and r["first_block"] == G + Nn
    # ke <= ka + 1: no signal block
    for ke in (G + Nn, G + Nn + 1):
        r = both(wm, p, 0, G + Nn, ke, fin)
        assert r["n_signal"] == 0 and r["signal"] == 0 and r["ratio_q8"] == 0 and r["n_noise"] == Nn
    r = both(wm, p, 0, G + Nn, G + Nn + 2, fin)
    assert r["n_signal"] == 1 and r["signal"] == int(p[G + Nn + 1])
    # noise 0 under a signal: the ratio saturates; noise 0 under signal 0: 0
    z = p.copy(); z[:Nn] = 0
    r = both(wm, z, 0, G + Nn, G + Nn + 5, fin)
    assert r["noise"] == 0 and r["signal"] > 0 and r["ratio_q8"] == PW.U32
    r = both(wm, np.zeros(p.size, np.uint32), 0, G + Nn, G + Nn + 5, fin)
    assert r["ratio_q8"] == 0 and r["n_signal"] == 4
    # the lower quartile: three quarters of the window may hold other telegrams
    q = p.copy(); q[Nn // 4 + 1:Nn] = 4000000000
    r = both(wm, q, 0, G + Nn, G + Nn + 5, fin)
    assert r["noise"] < 2000
    # a saturated ratio from finite numbers
    s = p.copy(); s[:Nn] = 1; s[G + Nn + 1:G + Nn + 5] = 4000000000
    r = both(wm, s, 0, G + Nn, G + Nn + 5, fin)
    assert r["noise"] == 1 and r["signal"] == 4000000000 and r["ratio_q8"] == PW.U32
    s[:Nn] = 300
    r = both(wm, s, 0, G + Nn, G + Nn + 5, fin)
    assert r["ratio_q8"] == 4000000000 * 256 // 300 < PW.U32
    # a timeline that starts inside the stream: the level blocks in front of it are missing
    r = both(wm, p[10:], 10, G + Nn, G + Nn + 5, fin)
    assert r["n_noise"] == Nn - 10


def test_more_signal_blocks_than_the_field_holds(wm):
    """70 000 signal blocks: n_signal stops at 65535, the mean is over all of them."""
    fin = 1600000
    G, Nn = PW.guard(fin)
    p = np.full(G + Nn + 70002, 7, np.uint32)
    p[G + Nn + 1:] = np.arange(70001, dtype=np.uint32) * 50000
    r = both(wm, p, 0, G + Nn, G + Nn + 70001, fin)
    assert r["n_signal"] == 65535 and r["signal"] == sum(range(70000)) * 50000 // 70000 and r["n_noise"] == Nn


def test_level_block_of_a_decimated_sample(wm):
    """m(n) = floor(n D M / L) >> 9 at the native rate, for other decimations and behind the resampler: 2.048 -> 1.6 MS/s is L / M = 25 / 32,
    2.5 -> 1.6 MS/s is 16 / 25; samples beyond 2^32 and 2^53."""
    assert PW.ratio_lm(2048000, 1600000) == (25, 32) and PW.ratio_lm(2500000, 1600000) == (16, 25)
    rng = np.random.default_rng(5)
    samples = [0, 1, 255, 256, 257, 799999, (1 << 32) + 12345, (1 << 53) + 1, (1 << 60) + 7] + [int(v) for v in rng.integers(0, 1 << 40, 200)]
    for d, rate in ((2, 0), (2, 1600000), (1, 0), (5, 0), (2, 2048000), (2, 2500000), (1, 1000000), (3, 10000000)):
        L, M = PW.ratio_lm(rate, d * 800000) if rate else (1, 1)
        assert (L, M) == tuple(wm.resampler_design(rate, d * 800000)[:2]) if rate and rate != d * 800000 else (L, M) == (1, 1)
        for n in samples:
            assert wm.line_power_block(n, d, rate) == PW.block_of(n, d, L, M), (d, rate, n)
    # an access code at decimated sample 100000 of a 2.048 MS/s capture: input sample 256000 exactly, block 500
    assert wm.line_power_block(100000, 2, 2048000) == 500 and wm.line_power_block(99999, 2, 2048000) == 499
    with pytest.raises(wm.WmbusError):
        wm.line_power_block(1, 2, 1234567)
    with pytest.raises(wm.WmbusError):
        wm.line_power_block(1, 0, 0)


@pytest.mark.parametrize("fin", RATES)
def test_window_of_the_shared_helper_equals_the_restatement(fin):
    """W, nb, cb, lo, j0 from wm_k0_power.h (what k0_channel_power and the host compute) for centres 0, +-Fin / 2, +-325 kHz, one Hz either
    side of every band edge near them, with the -s offsets on top, and random ones; and the properties the contract states: the window of
    W bins lies inside the nb bands whatever its alignment."""
    emu = load_emu()
    W, nb = PW.window(fin)
    assert (W, nb) == {800000: (128, 9), 1600000: (64, 5), 2400000: (42, 4), 4000000: (25, 3), 10000000: (10, 2)}[fin]
    centres = {0, fin // 2, -(fin // 2), 325000, -325000, fin // 2 + 325000, -(fin // 2) - 325000}
    for j in range(33):                                          # band edge j lies at (16 j - 256) Fin / 512: the Hz around the centres whose window starts there
        edge = (16 * j - 256 + W // 2) * fin // 512
        centres |= {edge - 1, edge, edge + 1, edge + fin // 1024 - 1, edge + fin // 1024, edge + fin // 1024 + 1}
    centres |= {int(v) for v in np.random.default_rng(fin).integers(-fin, fin, 200)}
    seen = set()
    for f in sorted(centres):
        out = (ctypes.c_int64 * 5)()
        emu.wm_emu_pow_window(fin, f, out)
        cb, lo, j0 = PW.centre(fin, f)
        assert list(out) == [W, nb, cb, lo, j0], (fin, f)
        assert 0 <= lo <= 512 - W and 0 <= j0 <= 32 - nb and 16 * j0 <= lo and lo + W <= 16 * (j0 + nb), (fin, f)
        seen.add(j0)
    assert PW.centre(fin, 0)[0] == 256 and PW.centre(fin, fin // 2)[0] == 512 and PW.centre(fin, -(fin // 2))[0] == 0
    assert seen == set(range(32 - nb + 1))
