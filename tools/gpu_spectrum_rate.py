#!/usr/bin/env python3
"""What the channel survey (cfg.input_spectrum) costs: ONE context of `--streams` (64) captures at 1.6 MS/s, pushes of 2^22 samples per
capture, HBM-resident (staged once, pushed again and again), with and without the field.  The two contexts live side by side in one
process and take turns: `--reps` (>= 5) repetitions each, interleaved without / with / without / ..., every repetition `--steps` timed
pushes after `--warmup` untimed ones at the start (one box visit, interleaved, the median and the spread).

Prints one JSON line per repetition -- samples/s of the repetition by the wall clock (process + collect of every push), the median
wmbus_timing.demod_ms of its pushes (the survey's kernel lies inside it) and gpu_total_ms -- and one summary line per leg: the median and
the smallest and largest samples/s over the repetitions, and the difference of the demod_ms medians, which is the kernel's time per push.

--format cu8|cs8|cs16|cf32 and --dc R measure the survey behind the other loaders and behind the DC blocker's table; both legs then run
the same conversion stage.  Kernel times proper: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o spectrum --output-format csv -- python tools/gpu_spectrum_rate.py --reps 1 --steps 3
and read the k0_spectrum<fmt, dc> row; a call reads streams x 2^22 x bytes per sample."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
wm = importlib.import_module("rtl-wmbus_amd")
import format_ref as FR  # noqa: E402  (the embeddings; the bytes are not checked here)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--format", default="cu8", choices=["cu8", "cs8", "cs16", "cf32"])
ap.add_argument("--dc", type=int, default=0, help="cfg.input_dc of both legs")
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_spectrum_rate.py: no HIP device")
n = 1 << a.log2_samples
fmt = {"cu8": FR.CU8, "cs8": FR.CS8, "cs16": FR.CS16, "cf32": FR.CF32}[a.format]
nbytes = FR.BPS[fmt] * n

caps = [FR.embed(wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0)[0], fmt) for s in range(a.distinct)]
legs = {}
for name, spectrum in (("without", 0), ("with", 1)):
    rx = wm.Receiver(n_streams=a.streams, max_push_bytes=nbytes, keep_taps=False, input_format=fmt, input_dc=a.dc, input_spectrum=spectrum)
    for s in range(a.streams):
        rx.stage(s, caps[s % a.distinct])
    for _ in range(a.warmup):
        rx.process(nbytes); rx.collect()
    legs[name] = rx

rates, demods = {k: [] for k in legs}, {k: [] for k in legs}
for r in range(a.reps):
    for name, rx in legs.items():
        demod, total = [], []
        t0 = time.perf_counter()
        for _ in range(a.steps):
            rx.process(nbytes); rx.collect()
            tm = rx.timing()
            demod.append(tm["demod_ms"]); total.append(tm["gpu_total_ms"])
        dt = time.perf_counter() - t0
        rate = a.streams * n * a.steps / dt
        rates[name].append(rate); demods[name].append(statistics.median(demod))
        print(json.dumps(dict(leg=name, rep=r, format=a.format, input_dc=a.dc, streams=a.streams, samples_per_stream=n, steps=a.steps, seconds=round(dt, 4),
                              msamples_per_s=round(rate / 1e6, 1), demod_ms_median=round(statistics.median(demod), 4),
                              gpu_total_ms_median=round(statistics.median(total), 4))), flush=True)
for name in legs:
    print(json.dumps(dict(summary=name, reps=a.reps, msamples_per_s_median=round(statistics.median(rates[name]) / 1e6, 1),
                          msamples_per_s_min=round(min(rates[name]) / 1e6, 1), msamples_per_s_max=round(max(rates[name]) / 1e6, 1),
                          demod_ms_median=round(statistics.median(demods[name]), 4))), flush=True)
d = statistics.median(demods["with"]) - statistics.median(demods["without"])
print(json.dumps(dict(summary="survey", demod_ms_added=round(d, 4), raw_gbytes_per_s_of_the_kernel=round(a.streams * nbytes / d / 1e6, 1) if d > 0 else None,
                      blocks_surveyed=legs["with"].read_spectrum(0)[2])), flush=True)
for rx in legs.values():
    rx.close()
