#!/usr/bin/env python3
"""What the GPU resampler (cfg.input_rate_hz) costs: 128 captures x 2^22 raw samples, HBM-resident, through wmbus_batch,
`--steps` timed pushes per context after `--warmup`; once at 2.048 MS/s with input_rate_hz = 2048000 and once natively at
1.6 MS/s (input_rate_hz = 0) on captures of the same raw size, the two legs alternating `--rounds` times in one process.
Prints one JSON line per leg and round: raw input Msamples/s.  Needs a GPU.

    tools/gpu_resample_rate.py [--steps 20] [--warmup 3] [--rounds 2] [--legs resample,native] [--streams 128] [--distinct 16]

The resampler kernel's own time: `rocprofv3 --kernel-trace --stats -d DIR -o k0 --output-format csv -- python
tools/gpu_resample_rate.py --legs resample --rounds 1 --steps 5`, rows k0_resample and k1_demod2 of the kernel statistics."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wm = importlib.import_module("rtl-wmbus_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--legs", default="resample,native")
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_resample_rate.py: no HIP device")

n = 1 << a.log2_samples
LEGS = {"resample": dict(fs_khz=2048, input_rate_hz=2048000), "native": dict(fs_khz=1600, input_rate_hz=0)}
batches = {}
for leg in a.legs.split(","):
    kw = LEGS[leg]
    caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=kw["fs_khz"], kinds=7, frames_per_s=20.0)[0] for s in range(a.distinct)]
    b = wm.Batch(n_streams=a.streams, max_push_bytes=2 * n, input_rate_hz=kw["input_rate_hz"])
    for s in range(a.streams):
        b.stage(s, caps[s % a.distinct])
    b.run_resident(2 * n, a.warmup)
    batches[leg] = b
for r in range(a.rounds):
    for leg, b in batches.items():
        st = b.run_resident(2 * n, a.steps)
        print(json.dumps(dict(leg=leg, round=r, input_rate_hz=LEGS[leg]["input_rate_hz"], streams=a.streams, raw_samples_per_stream=n,
                              contexts=len(b.contexts), steps=a.steps, seconds=round(st["seconds"], 4), lines=st["lines"],
                              raw_msamples_per_s=round(st["samples"] / st["seconds"] / 1e6, 1))), flush=True)
for b in batches.values():
    b.close()
