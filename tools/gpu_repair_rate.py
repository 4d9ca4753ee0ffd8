#!/usr/bin/env python3
"""What CRC repair (cfg.crc_repair, the CLI's -x) costs: ONE context of `--streams` (128) captures at 1.6 MS/s, pushes of
2^`--log2-samples` (22) samples per capture, HBM-resident (staged once, pushed again and again), on two batches in one visit -- a CLEAN
one (amplitude 60 over noise of sigma 2: next to no subjects) and a NOISY one (amplitude 40 over sigma 30, near the discriminator's
threshold: most telegrams that decode fail a CRC, and noise alone yields access codes whose "telegrams" are subjects too) -- three legs
each, side by side in one process:
    off      crc_repair = 0: in every respect the context a library without the field opens (the parent commit is its yardstick:
             bench.py on both builds; `--legs off` under the profiler lists its kernels)
    levels   line_levels = 1: the stage the field switches on by itself (k3_levels, k3_level_tail, the level records)
    on       crc_repair = 1: k3_repair behind them
`--reps` (>= 5) repetitions each, interleaved off / levels / on / off / ..., every repetition `--steps` timed pushes after `--warmup`
untimed ones at the start (one box visit, interleaved, the median and the spread).

One live stream:  --streams 1 --log2-samples 16.

Prints one JSON line per repetition -- samples/s by the wall clock (process + collect of every push), the medians of wmbus_timing's
gather_ms (the burst, level and repair kernels lie inside it), gpu_total_ms and host_decode_ms -- one summary line per batch and leg, the
differences of the medians, and what the last push of the `on` leg repaired.  The kernel apart: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o repair --output-format csv -- python tools/gpu_repair_rate.py --reps 1 --steps 3
and read the k3_repair row."""
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

LEGS = {"off": dict(), "levels": dict(line_levels=1), "on": dict(crc_repair=1)}
BATCHES = {"clean": dict(amplitude=60.0, noise_sigma=2.0), "noisy": dict(amplitude=40.0, noise_sigma=30.0)}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--legs", default="off,levels,on")
ap.add_argument("--batches", default="clean,noisy")
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_repair_rate.py: no HIP device")
n = 1 << a.log2_samples
nbytes = 2 * n
KEYS = ("gather_ms", "gpu_total_ms", "host_decode_ms")

for batch in a.batches.split(","):
    caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0, **BATCHES[batch])[0] for s in range(min(a.distinct, a.streams))]
    legs = {}
    for name in a.legs.split(","):
        rx = wm.Receiver(n_streams=a.streams, max_push_bytes=nbytes, keep_taps=False, **LEGS[name])
        for s in range(a.streams):
            rx.stage(s, caps[s % len(caps)])
        for _ in range(a.warmup):
            rx.process(nbytes); rx.collect()
        legs[name] = rx
    rates, med, wall = {k: [] for k in legs}, {k: {q: [] for q in KEYS} for k in legs}, {k: [] for k in legs}
    for r in range(a.reps):
        for name, rx in legs.items():
            seen = {q: [] for q in KEYS}
            t0 = time.perf_counter()
            for _ in range(a.steps):
                rx.process(nbytes); rx.collect()
                tm = rx.timing()
                for q in KEYS:
                    seen[q].append(tm[q])
            dt = time.perf_counter() - t0
            rate = a.streams * n * a.steps / dt
            rates[name].append(rate); wall[name].append(1e3 * dt / a.steps)
            for q in KEYS:
                med[name][q].append(statistics.median(seen[q]))
            print(json.dumps(dict(batch=batch, leg=name, rep=r, streams=a.streams, samples_per_stream=n, steps=a.steps, seconds=round(dt, 4),
                                  push_ms=round(1e3 * dt / a.steps, 4), msamples_per_s=round(rate / 1e6, 1),
                                  **{q + "_median": round(statistics.median(seen[q]), 4) for q in KEYS})), flush=True)
    for name in legs:
        print(json.dumps(dict(summary=name, batch=batch, reps=a.reps, msamples_per_s_median=round(statistics.median(rates[name]) / 1e6, 1),
                              msamples_per_s_min=round(min(rates[name]) / 1e6, 1), msamples_per_s_max=round(max(rates[name]) / 1e6, 1),
                              push_ms_median=round(statistics.median(wall[name]), 4),
                              **{q + "_median": round(statistics.median(med[name][q]), 4) for q in KEYS})), flush=True)
    first = next(iter(legs))
    for name in legs:
        if name != first:
            print(json.dumps(dict(summary="cost", batch=batch, leg=name, over=first,
                                  push_ms_added=round(statistics.median(wall[name]) - statistics.median(wall[first]), 4),
                                  **{q + "_added": round(statistics.median(med[name][q]) - statistics.median(med[first][q]), 4) for q in KEYS})), flush=True)
    if "on" in legs:                                         # what the last push held: lines, subjects, repaired
        reps = legs["on"].line_repairs()
        sub = [x for x in reps if x["blocks_bad"]]
        print(json.dumps(dict(summary="last push", batch=batch, lines=len(reps), subjects=len(sub),
                              repaired=sum(x["blocks_repaired"] == x["blocks_bad"] for x in sub), chips_flipped=sum(x["chips_flipped"] for x in sub if x["blocks_repaired"] == x["blocks_bad"]))), flush=True)
    for rx in legs.values():
        rx.close()
