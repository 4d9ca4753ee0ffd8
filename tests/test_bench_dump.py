"""bench.py --dump-outputs: the last push's lines of every context as .npy files (float64 / float32), within the size
budget, the same files for the same lines.  CPU only: the contexts are stand-ins that hand out lines like Receiver.lines()."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakeContext:
    def __init__(self, lines):
        self._lines = lines

    def lines(self):
        return self._lines


class FakeBatch:
    """Two contexts of four captures; capture s prints s % 3 lines (context-local stream numbers, as Receiver.lines())."""
    def __init__(self):
        self.contexts = []
        for first in (0, 4):
            lines = [dict(stream=k, chain=(first + k) % 2, algo=j % 2, crc_ok=int(j == 0), sample=(1 << 40) + 1000 * (first + k) + j,
                          text=f"t2a;T1;1;1;TS;{first + k};{j};0x{first + k:04x}{'ab' * j}\n")
                     for k in range(4) for j in range((first + k) % 3)]
            self.contexts.append((FakeContext(lines), first, 4))


def load_dir(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_line_as_float_arrays(tmp_path):
    bench = load_bench()
    rec = bench.dump_outputs(FakeBatch(), 8, str(tmp_path / "all"))
    got = load_dir(tmp_path / "all")
    assert set(got) == {"captures", "datagram_capture", "datagram_chain", "datagram_algo", "datagram_crc_ok", "datagram_sample",
                        "datagram_text_offset", "datagram_text"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    want = [(s, ln) for rx, first, _n in FakeBatch().contexts for ln in rx.lines() for s in [first + ln["stream"]]]
    assert rec["captures"] == 8 and rec["lines"] == len(want) and got["captures"].tolist() == list(range(8))
    assert got["datagram_capture"].tolist() == [s for s, _ln in want]
    assert got["datagram_sample"].tolist() == [ln["sample"] for _s, ln in want]
    off, text = got["datagram_text_offset"].astype(np.int64), got["datagram_text"].astype(np.uint8).tobytes()
    assert [text[off[k]:off[k + 1]].decode() for k in range(len(want))] == [ln["text"] for _s, ln in want]


def test_dump_outputs_samples_captures_within_the_budget(tmp_path):
    bench = load_bench()
    budget = 8 * 128 + 700
    a = bench.dump_outputs(FakeBatch(), 8, str(tmp_path / "a"), budget=budget)
    b = bench.dump_outputs(FakeBatch(), 8, str(tmp_path / "b"), budget=budget)
    assert 0 < a["captures"] < 8 and a == dict(b, dir=a["dir"])
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", n)) for n in os.listdir(tmp_path / "a")) <= budget
    ga, gb = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    assert set(ga["datagram_capture"].tolist()) <= set(ga["captures"].tolist())
