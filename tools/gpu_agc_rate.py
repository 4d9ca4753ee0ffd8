#!/usr/bin/env python3
"""What the per-block AGC (cfg.input_agc) costs: 128 captures x 2^22 raw samples, HBM-resident, through wmbus_batch, `--steps` timed
pushes per context after `--warmup`, all legs alternating `--rounds` times in one process (one box visit,
interleaved).  Legs, each with a fixed gain (input_gain_q8 = --gain-q8, default x 64: the K0 stage there was) and with input_agc = 1
(k0_agc_gain in front of the AG instantiation of the same stage):

    cu8 cs8 cs16 cf32   weak captures at 1.6 MS/s in the format: the conversion kernel
    rs25-cs16           cs16 at 2.5 MS/s: the resampler

The captures are a cu8 synthetic capture scaled down by --weak (default 16) around mid-scale, so that x 64 and the AGC both have work.
Prints one JSON line per leg and round: the mean and the median wmbus_timing.demod_ms over the round's pushes (the K0 stage and the gain
kernel lie inside it), raw input Msamples/s of the job, the clipped share.  The comparison is the same leg with the fixed gain in the
same process; --parent-lib adds `parent-cu8`, the plain path (no K0 stage) on another build of the library (the parent commit's), next
to `plain-cu8`, the same on this build.

Kernel times: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o agc --output-format csv -- python tools/gpu_agc_rate.py --rounds 1 --steps 5
and then `python tools/gpu_agc_rate.py --kernel-stats DIR/.../agc_kernel_stats.csv` (no GPU needed) prints, for every k0_agc_gain<fmt, dc>
row, the achieved bytes/s against the raw bytes a call reads (captures of a context x samples x bytes per sample), and the K0 rows
beside it."""
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
ap.add_argument("--legs", default="cu8,cs8,cs16,cf32,rs25-cs16")
ap.add_argument("--gain-q8", type=int, default=64 * 256)
ap.add_argument("--weak", type=int, default=16, help="the cu8 captures are scaled down by this around mid-scale")
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--parent-lib", default=None, help="libwmbus_hip.so of the parent commit (leg parent-cu8; skipped without it)")
ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel statistics CSV of a run of this tool: print the kernels' rates and exit")
a = ap.parse_args()
n = 1 << a.log2_samples
BPS = {"0": 2, "1": 2, "2": 4, "3": 8}                  # template argument FMT of k0_agc_gain -> raw bytes per sample

if a.kernel_stats:
    contexts = len(wm.batch_plan(a.streams))
    per_ctx = a.streams // contexts
    for row in csv.DictReader(open(a.kernel_stats)):
        name = row["Name"]
        if not re.search(r"k0_|k1_demod", name):
            continue
        out = dict(kernel=name, calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 1))
        m = re.search(r"k0_agc_gain<(\d)", name)
        if m:
            nbytes = per_ctx * n * BPS[m.group(1)]
            out.update(raw_bytes_per_call=nbytes, read_gb_per_s=round(nbytes / float(row["AverageNs"]), 1))
        print(json.dumps(out), flush=True)
    sys.exit(0)

if wm.device_count() < 1:
    sys.exit("gpu_agc_rate.py: no HIP device")


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


synth = {}
FORMATS = {"cu8": FR.CU8, "cs8": FR.CS8, "cs16": FR.CS16, "cf32": FR.CF32}


def capture(fs_khz, s, fmt):
    """Capture s at fs_khz, scaled down around mid-scale, in the format (cs16 / cf32: 128 x and 1 / 256 x of the cu8 sample x)."""
    key = (fs_khz, s)
    if key not in synth:
        cu8 = wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=fs_khz, kinds=7, frames_per_s=20.0)[0]
        synth[key] = (128 + (cu8.astype(np.int16) - 128) // a.weak).astype(np.uint8)
    return FR.embed(synth[key], fmt)


batches, meta = {}, {}
for leg in a.legs.split(",") + ["plain-cu8"] + (["parent-cu8"] if a.parent_lib else []):
    for agc in (0,) if leg.endswith("-cu8") else (0, 1):
        mod, kw, fs, fmt = wm, {}, 1600, FR.CU8
        if leg == "rs25-cs16":
            fs, fmt, kw = 2500, FR.CS16, dict(input_rate_hz=2500000, input_format=FR.CS16)
        elif leg == "parent-cu8":
            mod = second_copy(a.parent_lib)
        elif leg in FORMATS:
            fmt = FORMATS[leg]
            kw = dict(input_format=fmt)
        elif leg != "plain-cu8":
            sys.exit(f"gpu_agc_rate.py: unknown leg {leg}")
        if agc:
            kw.update(input_agc=1)
        elif not leg.endswith("-cu8"):
            kw.update(input_gain_q8=a.gain_q8)
        bps = FR.BPS[fmt]
        b = mod.Batch(n_streams=a.streams, max_push_bytes=bps * n, **kw)
        for s in range(a.streams):
            b.stage(s, capture(fs, s % a.distinct, fmt))
        b.run_resident(bps * n, a.warmup)
        name = f"{leg}+agc" if agc else leg
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
