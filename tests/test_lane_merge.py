"""The merge a batch lane orders its two contexts' stream operations with (rtl-wmbus_amd/csrc/wm_lane_merge.h, no HIP in it), on the
host: tests/lane_merge_check.cpp over 40 000 random pairs of operation lists -- each list's order kept, a permutation of both, exactly
the equal pairable heads paired, plain concatenation where nothing is pairable; no operation of the mate inside a K1 turn (given that
nothing pairable is recorded inside one); and the lists of real pushes in every variant: every launch that can pair does."""
import os
import subprocess

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


def test_lane_merge_keeps_order_and_pairs_equal_heads(tmp_path):
    exe = str(tmp_path / "lane_merge_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "rtl-wmbus_amd", "csrc"), "-o", exe, os.path.join(HERE, "lane_merge_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith(" 0 wrong"), p.stdout + p.stderr
    assert int(p.stdout.split()[0]) > 80000
