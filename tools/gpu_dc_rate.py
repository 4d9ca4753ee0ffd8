#!/usr/bin/env python3
"""What the I/Q DC blocker (cfg.input_dc) costs: 128 captures x 2^22 raw samples, HBM-resident, through wmbus_batch, `--steps` timed
pushes per context after `--warmup`, all legs alternating `--rounds` times in one process (one box visit,
interleaved).  Legs, each with input_dc = 0 and input_dc = --dc (default 6):

    cu8        cu8 at 1.6 MS/s: without the blocker no K0 stage at all, with it k0_dc_sums -> k0_dc_plan -> the conversion kernel
    rs25-cs16  cs16 at 2.5 MS/s, 6 bits down, gain 64: the resampler, without and with the two kernels in front of it

Prints one JSON line per leg and round: the mean and the median wmbus_timing.demod_ms over the round's pushes (the K0 stage and its two
DC kernels lie inside it), raw input Msamples/s of the job, the clipped share.  The comparison is the same leg without the blocker in
the same process; --parent-lib adds `parent-cu8`, the plain path on another build of the library (the parent commit's).

Kernel times: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o dc --output-format csv -- python tools/gpu_dc_rate.py --rounds 1 --steps 5
and then `python tools/gpu_dc_rate.py --kernel-stats DIR/.../dc_kernel_stats.csv` (no GPU needed) prints, for every k0_dc_sums<fmt>
row, the achieved bytes/s against the raw bytes a call reads (captures of a context x samples x bytes per sample), and the
k0_dc_plan and K0 rows beside it."""
import argparse
import csv
import importlib
import importlib.util
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
wm = importlib.import_module("rtl-wmbus_amd")
import format_ref as FR  # noqa: E402  (the embeddings; the bytes are not checked here)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--legs", default="cu8,rs25-cs16")
ap.add_argument("--dc", type=int, default=6)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--offset", default="12,-9", help="I/Q offset added to the cu8 captures, in cu8 steps")
ap.add_argument("--parent-lib", default=None, help="libwmbus_hip.so of the parent commit (leg parent-cu8; skipped without it)")
ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel statistics CSV of a run of this tool: print the kernels' rates and exit")
a = ap.parse_args()
n = 1 << a.log2_samples
BPS = {"0": 2, "1": 2, "2": 4, "3": 8}                  # template argument FMT of k0_dc_sums -> raw bytes per sample

if a.kernel_stats:
    contexts = len(wm.batch_plan(a.streams))
    per_ctx = a.streams // contexts
    for row in csv.DictReader(open(a.kernel_stats)):
        name = row["Name"]
        if not re.search(r"k0_|k1_demod", name):
            continue
        out = dict(kernel=name, calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 1))
        m = re.search(r"k0_dc_sums<(\d)>", name)
        if m:
            nbytes = per_ctx * n * BPS[m.group(1)]
            out.update(raw_bytes_per_call=nbytes, read_gb_per_s=round(nbytes / float(row["AverageNs"]), 1))
        print(json.dumps(out), flush=True)
    sys.exit(0)

if wm.device_count() < 1:
    sys.exit("gpu_dc_rate.py: no HIP device")


def second_copy(lib_path):
    """The package again, bound to another build of the library (with the __init__.py of that build where one lies next to the
    library: a build of another commit lays wmbus_cfg out differently)."""
    os.environ["WMBUS_HIP_LIB"] = lib_path
    mirror = os.path.join(os.path.dirname(os.path.abspath(lib_path)), "__init__.py")
    spec = importlib.util.spec_from_file_location("wm_parent", mirror if os.path.exists(mirror) else os.path.join(ROOT, "rtl-wmbus_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    del os.environ["WMBUS_HIP_LIB"]
    return mod


d_i, d_q = (int(v) for v in a.offset.split(","))
synth = {}


def capture(fs_khz, s, fmt):
    key = (fs_khz, s)
    if key not in synth:
        cu8 = wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=fs_khz, kinds=7, frames_per_s=20.0)[0]
        u = cu8.reshape(-1, 2).astype(np.int16) + np.array([d_i, d_q], np.int16)
        synth[key] = np.clip(u, 0, 255).astype(np.uint8).reshape(-1)
    raw = FR.embed(synth[key], fmt)
    return FR.raw_bytes(raw.view("<i2") >> 6, fmt) if fmt == FR.CS16 else raw


batches, meta = {}, {}
for leg in a.legs.split(",") + (["parent-cu8"] if a.parent_lib else []):
    for dc in (0,) if leg.startswith("parent") else (0, a.dc):
        mod, kw, fs, fmt = wm, {}, 1600, FR.CU8
        if leg == "rs25-cs16":
            fs, fmt, kw = 2500, FR.CS16, dict(input_rate_hz=2500000, input_format=FR.CS16, input_gain_q8=64 * 256)
        elif leg == "parent-cu8":
            mod = second_copy(a.parent_lib)
        elif leg != "cu8":
            sys.exit(f"gpu_dc_rate.py: unknown leg {leg}")
        if dc:
            kw.update(input_dc=dc)
        bps = FR.BPS[fmt]
        b = mod.Batch(n_streams=a.streams, max_push_bytes=bps * n, **kw)
        for s in range(a.streams):
            b.stage(s, capture(fs, s % a.distinct, fmt))
        b.run_resident(bps * n, a.warmup)
        name = f"{leg}+dc{dc}" if dc else leg
        batches[name], meta[name] = b, dict(fmt=FR.NAMES[fmt], bytes_per_sample=bps, fs_khz=fs, **{k: int(v) for k, v in kw.items()})
for r in range(a.rounds):
    for leg, b in batches.items():
        clip, demod = [0, 0], []

        def on_push(first, k, lines, tm, clip=clip, demod=demod):
            clip[0] += tm.get("input_clipped", 0); clip[1] += tm.get("input_bytes_out", 0)
            demod.append(tm["demod_ms"])
        st = b.run_resident(meta[leg]["bytes_per_sample"] * n, a.steps, on_push=on_push, want_lines=False)
        print(json.dumps(dict(leg=leg, round=r, **meta[leg], streams=a.streams, raw_samples_per_stream=n, contexts=len(b.contexts), steps=a.steps,
                              demod_ms_mean=round(statistics.mean(demod), 4), demod_ms_median=round(statistics.median(demod), 4), pushes=len(demod),
                              seconds=round(st["seconds"], 4), lines=st["lines"], raw_msamples_per_s=round(st["samples"] / st["seconds"] / 1e6, 1),
                              clipped_share=(clip[0] / clip[1] if clip[1] else None))), flush=True)
for b in batches.values():
    b.close()
