#!/usr/bin/env python3
"""What line quality (cfg.line_quality, the CLI's -q) costs: ONE context per leg, HBM-resident captures (staged once, pushed again and
again), in the two shapes of gpu_repair_rate.py -- the BATCH shape (128 captures at 1.6 MS/s, pushes of 2^22 samples per capture) and
the LIVE shape (one stream, pushes of 2^16 samples: 41 ms) -- each on a CLEAN synthetic batch (amplitude 60 over noise of sigma 2) and a
NOISY one (amplitude 40 over sigma 30, near the discriminator's threshold: noise alone yields access codes whose "telegrams" are
subjects too), two legs side by side in one process:
    off      line_quality = 0: in every respect the context a library without the field opens -- the parent commit's launch sequence
    on       line_quality = 1: the level stage the field switches on by itself (k3_levels, k3_level_tail) and k3_quality behind it
`--reps` (>= 5) repetitions each, interleaved off / on / off / ..., every repetition `--steps` timed pushes after `--warmup` untimed
ones at the start (one box visit, interleaved, the median and the spread).

Prints one JSON line per repetition -- samples/s by the wall clock (process + collect of every push), the medians of wmbus_timing's
gather_ms (the burst, level and quality kernels lie inside it), gpu_total_ms and host_decode_ms -- one summary line per shape, batch and
leg, the differences of the medians, and what the last push of the `on` leg measured.  The kernel apart: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o quality --output-format csv -- python tools/gpu_quality_rate.py --reps 1 --steps 3
and read the k3_quality row."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wm = importlib.import_module("rtl-wmbus_amd")

LEGS = {"off": dict(), "on": dict(line_quality=1)}
BATCHES = {"clean": dict(amplitude=60.0, noise_sigma=2.0), "noisy": dict(amplitude=40.0, noise_sigma=30.0)}
SHAPES = {"batch": (128, 22), "live": (1, 16)}                # streams, log2 of the samples per push and stream

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--legs", default="off,on")
ap.add_argument("--batches", default="clean,noisy")
ap.add_argument("--shapes", default="batch,live")
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_quality_rate.py: no HIP device")
KEYS = ("gather_ms", "gpu_total_ms", "host_decode_ms")

for shape in a.shapes.split(","):
    streams, log2_samples = SHAPES[shape]
    n = 1 << log2_samples
    nbytes = 2 * n
    steps = a.steps * (8 if shape == "live" else 1)              # a live push is short: more of them per repetition
    for batch in a.batches.split(","):
        caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0 if shape == "batch" else 100.0, **BATCHES[batch])[0]
                for s in range(min(a.distinct, streams))]
        legs = {}
        for name in a.legs.split(","):
            rx = wm.Receiver(n_streams=streams, max_push_bytes=nbytes, keep_taps=False, **LEGS[name])
            for s in range(streams):
                rx.stage(s, caps[s % len(caps)])
            for _ in range(a.warmup):
                rx.process(nbytes); rx.collect()
            legs[name] = rx
        rates, med, wall = {k: [] for k in legs}, {k: {q: [] for q in KEYS} for k in legs}, {k: [] for k in legs}
        for r in range(a.reps):
            for name, rx in legs.items():
                seen = {q: [] for q in KEYS}
                t0 = time.perf_counter()
                for _ in range(steps):
                    rx.process(nbytes); rx.collect()
                    tm = rx.timing()
                    for q in KEYS:
                        seen[q].append(tm[q])
                dt = time.perf_counter() - t0
                rate = streams * n * steps / dt
                rates[name].append(rate); wall[name].append(1e3 * dt / steps)
                for q in KEYS:
                    med[name][q].append(statistics.median(seen[q]))
                print(json.dumps(dict(shape=shape, batch=batch, leg=name, rep=r, streams=streams, samples_per_stream=n, steps=steps, seconds=round(dt, 4),
                                      push_ms=round(1e3 * dt / steps, 4), msamples_per_s=round(rate / 1e6, 1),
                                      **{q + "_median": round(statistics.median(seen[q]), 4) for q in KEYS})), flush=True)
        for name in legs:
            print(json.dumps(dict(summary=name, shape=shape, batch=batch, reps=a.reps, msamples_per_s_median=round(statistics.median(rates[name]) / 1e6, 1),
                                  msamples_per_s_min=round(min(rates[name]) / 1e6, 1), msamples_per_s_max=round(max(rates[name]) / 1e6, 1),
                                  push_ms_median=round(statistics.median(wall[name]), 4), push_ms_min=round(min(wall[name]), 4), push_ms_max=round(max(wall[name]), 4),
                                  **{q + "_median": round(statistics.median(med[name][q]), 4) for q in KEYS})), flush=True)
        first = next(iter(legs))
        for name in legs:
            if name != first:
                print(json.dumps(dict(summary="cost", shape=shape, batch=batch, leg=name, over=first,
                                      push_ms_added=round(statistics.median(wall[name]) - statistics.median(wall[first]), 4),
                                      **{q + "_added": round(statistics.median(med[name][q]) - statistics.median(med[first][q]), 4) for q in KEYS})), flush=True)
        if "on" in legs:                                         # what the last push held: lines, measured, closed eyes
            recs = legs["on"].line_quality()
            got = [x for x in recs if x["n"]]
            print(json.dumps(dict(summary="last push", shape=shape, batch=batch, lines=len(recs), measured=len(got), closed_eye=sum(x["eye_hz"] <= 0 for x in got),
                                  chips=sum(x["n"] for x in got))), flush=True)
        for rx in legs.values():
            rx.close()
