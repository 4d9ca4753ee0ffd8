#!/usr/bin/env python3
"""What channel power (cfg.line_power) costs: ONE context of `--streams` (64) captures at 1.6 MS/s, pushes of 2^22 samples per capture,
HBM-resident (staged once, pushed again and again), three legs side by side in one process: without anything, with the plain survey
(cfg.input_spectrum) and with cfg.line_power -- the band form of the survey, k0_channel_power and its copy to the host.  `--reps` (>= 5)
repetitions each, interleaved without / spectrum / power / without / ..., every repetition `--steps` timed pushes after `--warmup`
untimed ones at the start (one box visit, interleaved, the median and the spread).

Prints one JSON line per repetition -- samples/s by the wall clock (process + collect of every push), the median wmbus_timing.demod_ms of
its pushes (the survey's kernels lie inside it), gather_ms (line_power switches the level kernels on) and host_decode_ms (the records) --
one summary line per leg, and the differences of the demod_ms medians: the plain survey's time per push, and what the bands and
k0_channel_power add to it.  The two kernels apart: run once under the profiler,
    rocprofv3 --kernel-trace --stats -d DIR -o power --output-format csv -- python tools/gpu_power_rate.py --reps 1 --steps 3
and read the k0_spectrum<fmt, dc, age, true> and k0_channel_power rows."""
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
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_power_rate.py: no HIP device")
n = 1 << a.log2_samples
fmt = {"cu8": FR.CU8, "cs8": FR.CS8, "cs16": FR.CS16, "cf32": FR.CF32}[a.format]
nbytes = FR.BPS[fmt] * n

caps = [FR.embed(wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0)[0], fmt) for s in range(a.distinct)]
legs = {}
for name, kw in (("without", dict()), ("spectrum", dict(input_spectrum=1)), ("power", dict(line_power=1))):
    rx = wm.Receiver(n_streams=a.streams, max_push_bytes=nbytes, keep_taps=False, input_format=fmt, **kw)
    for s in range(a.streams):
        rx.stage(s, caps[s % a.distinct])
    for _ in range(a.warmup):
        rx.process(nbytes); rx.collect()
    legs[name] = rx

KEYS = ("demod_ms", "gather_ms", "host_decode_ms", "gpu_total_ms")
rates, med = {k: [] for k in legs}, {k: {q: [] for q in KEYS} for k in legs}
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
        rates[name].append(rate)
        for q in KEYS:
            med[name][q].append(statistics.median(seen[q]))
        print(json.dumps(dict(leg=name, rep=r, format=a.format, streams=a.streams, samples_per_stream=n, steps=a.steps, seconds=round(dt, 4),
                              msamples_per_s=round(rate / 1e6, 1), **{q + "_median": round(statistics.median(seen[q]), 4) for q in KEYS})), flush=True)
for name in legs:
    print(json.dumps(dict(summary=name, reps=a.reps, msamples_per_s_median=round(statistics.median(rates[name]) / 1e6, 1),
                          msamples_per_s_min=round(min(rates[name]) / 1e6, 1), msamples_per_s_max=round(max(rates[name]) / 1e6, 1),
                          **{q + "_median": round(statistics.median(med[name][q]), 4) for q in KEYS})), flush=True)
demod = {name: statistics.median(med[name]["demod_ms"]) for name in legs}
plain, banded = demod["spectrum"] - demod["without"], demod["power"] - demod["without"]
print(json.dumps(dict(summary="cost", survey_demod_ms_added=round(plain, 4), line_power_demod_ms_added=round(banded, 4),
                      bands_and_channel_power_ms=round(banded - plain, 4),
                      survey_raw_gbytes_per_s=round(a.streams * nbytes / plain / 1e6, 1) if plain > 0 else None,
                      band_form_raw_gbytes_per_s=round(a.streams * nbytes / banded / 1e6, 1) if banded > 0 else None,
                      records=len(legs["power"].line_power()), rows=int(legs["power"].read_waterfall(0)[0].shape[0]))), flush=True)
for rx in legs.values():
    rx.close()
