"""cfg.input_shift_hz in the ABI, and wmbus_shift_design (host only): the step against the Python integer formula, the table against
numpy, its quarter-turn symmetry, bad arguments.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import shift_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_abi_has_the_shift_field(wm):
    """Fails on a tree without the feature.  The field sits directly behind input_rate_hz, not at the end of the struct."""
    names = [f[0] for f in wm.Cfg._fields_]
    assert names[names.index("input_rate_hz") + 1] == "input_shift_hz"
    assert dict(wm.Cfg._fields_)["input_shift_hz"] is ctypes.c_int       # signed
    c = wm.Cfg()
    ctypes.memset(ctypes.byref(c), 0xFF, ctypes.sizeof(c))
    wm.lib().wmbus_default_cfg(ctypes.byref(c))
    assert c.input_shift_hz == 0 and c.input_rate_hz == 0
    assert wm._make_cfg(input_shift_hz=-123457).input_shift_hz == -123457
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "wmbus_hip.h")).read()
    for word in ("int input_shift_hz;", "wmbus_shift_design(unsigned in_hz, int shift_hz, uint32_t *step, int16_t *table, size_t cap)"):
        assert word in hdr, word
    assert hdr.index("unsigned input_rate_hz;") < hdr.index("int input_shift_hz;") < hdr.index("unsigned input_format;")


FINS = [800000, 1600000, 2048000, 2500000, 10000000, 3999999, 4294967295]


def cases():
    out = []
    for fin in FINS:
        for f in (0, 1, -1, fin // 2, -(fin // 2), 200000, -123457, fin // 4, -(fin // 3), fin // 2 - 1, 1 - fin // 2):
            out.append((fin, f))
    return out


def test_step_equals_the_integer_formula(wm):
    for fin, f in cases():
        want = ((f * 2 ** 32 + fin // 2) // fin) % 2 ** 32               # Python integers: // is floor division
        assert want == SR.step_of(fin, f)
        step = ctypes.c_uint32(0xDEADBEEF)
        assert wm.lib().wmbus_shift_design(fin, f, ctypes.byref(step), None, 0) == 0, (fin, f)
        assert step.value == want, (fin, f, step.value, want)
        assert wm.shift_design(fin, f)[0] == want
    assert wm.shift_design(1600000, 0)[0] == 0
    assert wm.shift_design(1600000, 800000)[0] == 2 ** 31 == wm.shift_design(1600000, -800000)[0]      # half a turn either way
    assert wm.shift_design(1600000, 400000)[0] == 2 ** 30 and wm.shift_design(1600000, -400000)[0] == 3 * 2 ** 30
    assert wm.shift_design(4294967295, -1)[0] == 2 ** 32 - 1 and wm.shift_design(4294967295, 1)[0] == 1


def test_table_equals_numpy_and_is_symmetric(wm):
    _, t = wm.shift_design(1600000, 200000)
    assert t.shape == (1024, 2) and t.dtype == np.int16
    w = 2.0 * np.pi * np.arange(1024) / 1024
    assert np.array_equal(t[:, 0], np.rint(16384 * np.cos(w)).astype(np.int16))
    assert np.array_equal(t[:, 1], np.rint(16384 * np.sin(w)).astype(np.int16))
    assert np.array_equal(t.astype(np.int64), SR.table())
    i = np.arange(1024)
    assert np.array_equal(t[(i + 256) % 1024, 0], -t[i, 1]) and np.array_equal(t[(i + 256) % 1024, 1], t[i, 0])      # entry i + 256 = {-s, c}
    assert t[0].tolist() == [16384, 0] and t[256].tolist() == [0, 16384] and t[512].tolist() == [-16384, 0] and t[768].tolist() == [0, -16384]
    assert np.abs(t.astype(np.int64)).sum(axis=1).max() <= 23171         # |c| + |s| <= 16384 sqrt 2: 32768 of it stays inside int32
    # the table does not depend on the arguments
    assert np.array_equal(wm.shift_design(4294967295, -7)[1], t)


def test_bad_arguments_are_refused(wm):
    L = wm.lib()
    step = ctypes.c_uint32()
    buf = np.zeros(2048, np.int16)
    EINVAL = -1
    for fin, f in ((1600000, 800001), (1600000, -800001), (1600001, 800001), (1600001, -800001), (800000, 2 ** 31 - 1), (4294967295, -2 ** 31),
                   (799999, 0), (0, 0), (799999, 1)):
        assert L.wmbus_shift_design(fin, f, ctypes.byref(step), None, 0) == EINVAL, (fin, f)
    assert L.wmbus_shift_design(1600001, 800000, ctypes.byref(step), None, 0) == 0                 # |f| <= Fin / 2 = 800000.5
    assert L.wmbus_shift_design(1600000, 1, ctypes.byref(step), buf.ctypes.data, 2047) == EINVAL   # the table needs 2048 int16
    assert L.wmbus_shift_design(1600000, 1, None, buf.ctypes.data, 2048) == 0 and buf[0] == 16384  # step may be NULL
    with pytest.raises(wm.WmbusError):
        wm.shift_design(1600000, 800001)
