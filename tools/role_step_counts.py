#!/usr/bin/env python3
"""Instructions in each role's step loop of a systolic clock kernel, from a plain device assembly listing:

    hipcc $(make -s -C rtl-wmbus_amd print-hipflags) -S --cuda-device-only -o wm.s rtl-wmbus_amd/csrc/wm_api.hip
    tools/role_step_counts.py wm.s [mangled kernel name ...]          (default: k2_clock_sys<false, true>, the product's first pass)

A step loop is a maximal run of code closed by a backward branch with an s_barrier in it; the four roles are told apart by what
their loops hold (f32 arithmetic, global loads and stores).  The step's cost is the critical role's count."""
import re
import sys


def step_loops(path, sym):
    text = open(path).read()
    m = re.search(r"^%s:.*?^\s*s_endpgm" % re.escape(sym), text, re.S | re.M)
    if not m:
        sys.exit("no kernel %s in %s" % (sym, path))
    ins, labels = [], {}
    for line in m.group(0).split("\n"):
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        if t.endswith(":"):
            labels[t[:-1]] = len(ins)
        else:
            ins.append(t)
    spans = []
    for i, t in enumerate(ins):
        b = re.match(r"s_c?branch\S*\s+(\S+)", t)
        if b and labels.get(b.group(1), i + 1) <= i and any("s_barrier" in u for u in ins[labels[b.group(1)]:i + 1]):
            spans.append([labels[b.group(1)], i])
    merged = []
    for a, b in sorted(spans):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    rows = []
    for a, b in merged:
        seg = ins[a:b + 1]
        n = lambda pat: sum(1 for t in seg if re.match(pat, t))
        f32, loads, stores = n(r"v_(mul|add|sub)_f32"), n(r"global_load"), n(r"global_(store|atomic)")
        role = 3 if stores else 1 if loads >= 8 else 0 if f32 > 450 else 2      # role 0 carries two variants of its block (warm-up, full) and the DC stage
        rows.append((role, len(seg), f32, loads, stores, n(r"ds_")))
    return len(ins), sorted(rows)


if __name__ == "__main__":
    for sym in sys.argv[2:] or ["_Z12k2_clock_sysILb0ELb1EEv6K2Args"]:
        total, rows = step_loops(sys.argv[1], sym)
        print("%s: %d instructions in the kernel" % (sym, total))
        for r in rows:
            print("    role %d step loop: %4d instructions (%3d f32 mul/add/sub, %2d global loads, %2d global stores/atomics, %2d LDS)" % r)
