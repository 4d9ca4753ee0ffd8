#!/usr/bin/env python3
"""What decoding C channels of one wideband capture in one context (cfg.input_channels) costs against C separate single-shift contexts:
`--captures` captures x 2^`--log2-samples` raw samples, HBM-resident, through wmbus_batch with ONE context, `--steps` timed pushes after
`--warmup`, all legs alternating `--rounds` times in one process (one box visit, interleaved).  Inputs:

    cs16-10M   cs16 at 10 MS/s (L / M = 4 / 25): the resampler
    cu8        cu8 at 1.6 MS/s: the conversion kernel

and for C = 1, 2, 4, 8 the legs

    <input>/chan-C     one context with input_channel_hz of C entries (pipeline width captures x C)
    <input>/single-C   C contexts with input_shift_hz = hz[c] each, run one after the other on the same input: their demod_ms and seconds
                       are summed.  With --parent-lib they are opened on that build of the library (the parent commit's) and the leg is
                       called parent-C.

Prints one JSON line per leg and round: the mean wmbus_timing.demod_ms per context-push (the K0 stage lies inside it; summed over the C
contexts of a single / parent leg), the job's seconds, decoded channel-samples per second, and the raw bytes a host source would stage
over PCIe per decoded channel (counted, not timed: the input is resident) -- raw bytes per capture / C for a channels context, raw bytes
per capture for separate contexts.

Kernel times: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o ch --output-format csv -- python tools/gpu_channels_rate.py --rounds 1 --steps 5
and read the k0_* rows of DIR/.../ch_kernel_stats.csv."""
import argparse
import importlib
import importlib.util
import json
import os
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
ap.add_argument("--inputs", default="cs16-10M,cu8")
ap.add_argument("--channels", default="1,2,4,8")
ap.add_argument("--captures", type=int, default=16)
ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--parent-lib", default=None, help="libwmbus_hip.so of the parent commit for the separate single-shift contexts")
ap.add_argument("--only", default="chan,single", help="leg kinds to run (a profiler run of one kind: --only chan)")
a = ap.parse_args()
n = 1 << a.log2_samples

if wm.device_count() < 1:
    sys.exit("gpu_channels_rate.py: no HIP device")


def second_copy(lib_path):
    """The package again, bound to another build of the library (with the __init__.py of that build where one lies next to the library:
    a build of another commit lays wmbus_cfg out differently)."""
    os.environ["WMBUS_HIP_LIB"] = lib_path
    mirror = os.path.join(os.path.dirname(os.path.abspath(lib_path)), "__init__.py")
    spec = importlib.util.spec_from_file_location("wm_parent", mirror if os.path.exists(mirror) else os.path.join(ROOT, "rtl-wmbus_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    del os.environ["WMBUS_HIP_LIB"]
    return mod


INPUTS = {"cs16-10M": (10000, FR.CS16, dict(input_rate_hz=10000000, input_format=FR.CS16, input_gain_q8=4096)),
          "cu8": (1600, FR.CU8, dict())}
synth = {}


def capture(fs_khz, s, fmt):
    if (fs_khz, s) not in synth:
        synth[(fs_khz, s)] = wm.synth_capture(seed=0xC4A7 + s, n_samples=n, fs_khz=fs_khz, kinds=7, frames_per_s=20.0)[0]
    return FR.embed(synth[(fs_khz, s)], fmt)


def offsets(fs_khz, C):
    """C offsets spread over +- 0.4 of the input rate, none 0 (a single-shift context with 0 is the plain path)."""
    return [int((c + 1) * (1 if c % 2 == 0 else -1) * 0.05 * fs_khz * 1000) for c in range(C)]


single_mod = second_copy(a.parent_lib) if a.parent_lib else wm
single_name = "parent" if a.parent_lib else "single"
legs, meta = {}, {}
for inp in a.inputs.split(","):
    fs, fmt, kw = INPUTS[inp]
    bps = FR.BPS[fmt]
    raw = [capture(fs, s % a.distinct, fmt) for s in range(a.captures)]
    for C in [int(c) for c in a.channels.split(",")]:
        hz = offsets(fs, C)
        kinds = []
        if "chan" in a.only:
            kinds.append((f"{inp}/chan-{C}", [wm.Batch(n_streams=a.captures, contexts=1, max_push_bytes=bps * n, input_channel_hz=hz, **kw)]))
        if "single" in a.only:
            kinds.append((f"{inp}/{single_name}-{C}", [single_mod.Batch(n_streams=a.captures, contexts=1, max_push_bytes=bps * n, input_shift_hz=f, **kw) for f in hz]))
        for name, batches in kinds:
            for b in batches:
                for s in range(a.captures):
                    b.stage(s, raw[s])
                b.run_resident(bps * n, a.warmup)
            legs[name] = batches
            meta[name] = dict(input=inp, channels=C, contexts=len(batches), bytes_per_sample=bps,
                              pcie_bytes_per_decoded_channel=bps * n * len(batches) // C)
for r in range(a.rounds):
    for name, batches in legs.items():
        demod, seconds, lines, clip = 0.0, 0.0, 0, [0, 0]
        for b in batches:
            ms = []

            def on_push(first, k, recs, tm, ms=ms, clip=clip):
                ms.append(tm["demod_ms"]); clip[0] += tm.get("input_clipped", 0); clip[1] += tm.get("input_bytes_out", 0)
            st = b.run_resident(meta[name]["bytes_per_sample"] * n, a.steps, on_push=on_push, want_lines=False)
            demod += statistics.mean(ms); seconds += st["seconds"]; lines += st["lines"]
        C = meta[name]["channels"]
        print(json.dumps(dict(leg=name, round=r, **meta[name], captures=a.captures, raw_samples_per_capture=n, steps=a.steps,
                              demod_ms_per_push=round(demod, 4), seconds=round(seconds, 4), lines=lines,
                              channel_msamples_per_s=round(a.captures * C * n * a.steps / seconds / 1e6, 1),
                              clipped_share=(clip[0] / clip[1] if clip[1] else None))), flush=True)
for batches in legs.values():
    for b in batches:
        b.close()
