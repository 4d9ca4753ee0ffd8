#!/usr/bin/env python3
"""What channel activity (cfg.channel_activity) costs on top of channel power: ONE context of `--streams` (128) captures at 1.6 MS/s,
pushes of 2^`--log2-samples` (22) samples per capture, HBM-resident (staged once, pushed again and again), two legs side by side in one
process: cfg.line_power = 1 -- in every respect the context a library without the field opens -- and cfg.channel_activity = 1, which adds
k0_activity behind k0_channel_power, the copy of its ticket count and, for a push that closed any burst, the copy of the records and their
sort.  `--reps` (>= 5) repetitions each, interleaved power / activity / power / ..., every repetition `--steps` timed pushes after
`--warmup` untimed ones at the start (one box visit, interleaved, the median and the spread).

One live stream:  --streams 1 --log2-samples 16  (a push of 41 ms of a 1.6 MS/s receiver).

Prints one JSON line per repetition -- samples/s by the wall clock (process + collect of every push), the median wmbus_timing.demod_ms of
its pushes (the input stage's kernels lie inside it) and gpu_total_ms -- one summary line per leg, and the differences of the medians.
The kernel apart: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o activity --output-format csv -- python tools/gpu_activity_rate.py --reps 1 --steps 3
and read the k0_activity row."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_activity_rate.py: no HIP device")
n = 1 << a.log2_samples
nbytes = 2 * n

caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0)[0] for s in range(min(a.distinct, a.streams))]
legs = {}
for name, kw in (("power", dict(line_power=1)), ("activity", dict(channel_activity=1))):
    rx = wm.Receiver(n_streams=a.streams, max_push_bytes=nbytes, keep_taps=False, **kw)
    for s in range(a.streams):
        rx.stage(s, caps[s % len(caps)])
    for _ in range(a.warmup):
        rx.process(nbytes); rx.collect()
    legs[name] = rx

KEYS = ("demod_ms", "gpu_total_ms", "host_decode_ms")
rates, med, wall = {k: [] for k in legs}, {k: {q: [] for q in KEYS} for k in legs}, {k: [] for k in legs}
bursts = 0
for r in range(a.reps):
    for name, rx in legs.items():
        seen = {q: [] for q in KEYS}
        t0 = time.perf_counter()
        for _ in range(a.steps):
            rx.process(nbytes); rx.collect()
            tm = rx.timing()
            for q in KEYS:
                seen[q].append(tm[q])
            if name == "activity":                               # the count alone: the mirror's dicts are not the library's cost
                bursts = int(wm.lib().wmbus_activity(rx._h, None))
        dt = time.perf_counter() - t0
        rate = a.streams * n * a.steps / dt
        rates[name].append(rate); wall[name].append(1e3 * dt / a.steps)
        for q in KEYS:
            med[name][q].append(statistics.median(seen[q]))
        print(json.dumps(dict(leg=name, rep=r, streams=a.streams, samples_per_stream=n, steps=a.steps, seconds=round(dt, 4), push_ms=round(1e3 * dt / a.steps, 4),
                              msamples_per_s=round(rate / 1e6, 1), **{q + "_median": round(statistics.median(seen[q]), 4) for q in KEYS})), flush=True)
for name in legs:
    print(json.dumps(dict(summary=name, reps=a.reps, msamples_per_s_median=round(statistics.median(rates[name]) / 1e6, 1),
                          msamples_per_s_min=round(min(rates[name]) / 1e6, 1), msamples_per_s_max=round(max(rates[name]) / 1e6, 1),
                          push_ms_median=round(statistics.median(wall[name]), 4), push_ms_min=round(min(wall[name]), 4), push_ms_max=round(max(wall[name]), 4),
                          **{q + "_median": round(statistics.median(med[name][q]), 4) for q in KEYS})), flush=True)
diff = {q: statistics.median(med["activity"][q]) - statistics.median(med["power"][q]) for q in KEYS}
print(json.dumps(dict(summary="cost", push_ms_added=round(statistics.median(wall["activity"]) - statistics.median(wall["power"]), 4),
                      **{q + "_added": round(v, 4) for q, v in diff.items()}, bursts_in_last_push=bursts, rows=2 * a.streams,
                      level_blocks_per_push=n // 512)), flush=True)
for rx in legs.values():
    rx.close()
