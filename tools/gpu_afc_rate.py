#!/usr/bin/env python3
"""What automatic frequency correction (cfg.input_afc) costs per push against its nearest equivalent without it: the same context with
cfg.input_spectrum = 1 and a fixed cfg.input_shift_hz (the survey and a rotating stage kernel run in both; AFC adds k0_afc_plan, one block
per capture, and the stage kernel reads its step from a table).  ONE context of `--streams` captures at 1.6 MS/s, pushes of
2^`--log2-samples` samples per capture, HBM-resident (staged once, pushed again and again).  The two contexts live side by side in one
process and take turns: `--reps` (>= 5) repetitions each, interleaved fixed / afc / fixed / ..., every repetition `--steps` timed pushes
after `--warmup` untimed ones at the start (one box visit, interleaved, the median and the spread).

The shapes DESIGN.md section 6 quotes: the bench's batch shape, --streams 64 --log2-samples 22 (the default), and a live stream's single
capture, --streams 1 --log2-samples 19 --steps 20.

Prints one JSON line per repetition -- the wall clock per push (process + collect), the median wmbus_timing.demod_ms of its pushes (every
K0 kernel lies inside it) and gpu_total_ms -- and one summary line per leg and one for the difference.  The fixed leg's shift is the lock
the AFC leg reports for capture 0 after its warm-up (1 Hz if that is 0: the rotating kernel, not the plain one).

Three more legs at the same shape, in the same interleaved order, each held against its counterpart of the same visit:
    afc_aged     AFC on a survey that forgets (cfg.input_spectrum_age = `--age`, default 16) against `afc`: the same transform, one more
                 flush per epoch edge inside a wave's run, a fill per newly entered epoch, and a plan kernel that reads two slots
    ch2_fixed    a list of two fixed channels (cfg.input_channel_hz = [lock, lock + 100000]) with the survey on
    ch2_afc      the same list with a lock per channel (cfg.input_channel_afc_hz = [64000, 64000]) against `ch2_fixed`: the plan kernel on
                 a grid of (captures, 2), the stage kernel's step from its table
--legs picks a subset (fixed and afc are always there).  Kernel times proper:
    rocprofv3 --kernel-trace --stats -d DIR -o afc --output-format csv -- python tools/gpu_afc_rate.py --reps 1 --steps 3
and read the k0_afc_plan row."""
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
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--age", type=int, default=16, help="cfg.input_spectrum_age of the afc_aged leg")
ap.add_argument("--legs", default="afc_aged,ch2_fixed,ch2_afc", help="the legs beside fixed and afc, comma separated (empty: none)")
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_afc_rate.py: no HIP device")
n = 1 << a.log2_samples
nbytes = 2 * n

caps = [wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=1600, kinds=7, frames_per_s=20.0)[0] for s in range(min(a.distinct, a.streams))]


def opened(**kw):
    rx = wm.Receiver(n_streams=a.streams, max_push_bytes=nbytes, keep_taps=False, **kw)
    for s in range(a.streams):
        rx.stage(s, caps[s % len(caps)])
    for _ in range(a.warmup):
        rx.process(nbytes); rx.collect()
    return rx


legs = {"afc": opened(input_afc=1)}
lock = legs["afc"].read_input_afc(0)
legs = {"fixed": opened(input_spectrum=1, input_shift_hz=lock["shift_hz"] or 1), "afc": legs["afc"]}
more = [x for x in a.legs.split(",") if x]
pair = [lock["shift_hz"] or 1, (lock["shift_hz"] or 1) + 100000]
if "afc_aged" in more:
    legs["afc_aged"] = opened(input_afc=1, input_spectrum_age=a.age)
if "ch2_fixed" in more:
    legs["ch2_fixed"] = opened(input_spectrum=1, input_channel_hz=pair)
if "ch2_afc" in more:
    legs["ch2_afc"] = opened(input_channel_hz=pair, input_channel_afc_hz=[64000, 64000])

push_ms, demods = {k: [] for k in legs}, {k: [] for k in legs}
for r in range(a.reps):
    for name, rx in legs.items():
        demod, total = [], []
        t0 = time.perf_counter()
        for _ in range(a.steps):
            rx.process(nbytes); rx.collect()
            tm = rx.timing()
            demod.append(tm["demod_ms"]); total.append(tm["gpu_total_ms"])
        dt = time.perf_counter() - t0
        push_ms[name].append(1e3 * dt / a.steps); demods[name].append(statistics.median(demod))
        print(json.dumps(dict(leg=name, rep=r, streams=a.streams, samples_per_stream=n, steps=a.steps, push_ms=round(1e3 * dt / a.steps, 4),
                              msamples_per_s=round(a.streams * n * a.steps / dt / 1e6, 1), demod_ms_median=round(statistics.median(demod), 4),
                              gpu_total_ms_median=round(statistics.median(total), 4))), flush=True)
for name in legs:
    print(json.dumps(dict(summary=name, reps=a.reps, push_ms_median=round(statistics.median(push_ms[name]), 4), push_ms_min=round(min(push_ms[name]), 4),
                          push_ms_max=round(max(push_ms[name]), 4), demod_ms_median=round(statistics.median(demods[name]), 4))), flush=True)
print(json.dumps(dict(summary="afc - fixed", push_ms=round(statistics.median(push_ms["afc"]) - statistics.median(push_ms["fixed"]), 4),
                      demod_ms=round(statistics.median(demods["afc"]) - statistics.median(demods["fixed"]), 4), lock=lock,
                      lock_at_the_end=legs["afc"].read_input_afc(0))), flush=True)
for name, against in (("afc_aged", "afc"), ("ch2_afc", "ch2_fixed")):
    if name in legs and against in legs:
        print(json.dumps(dict(summary=f"{name} - {against}", push_ms=round(statistics.median(push_ms[name]) - statistics.median(push_ms[against]), 4),
                              demod_ms=round(statistics.median(demods[name]) - statistics.median(demods[against]), 4),
                              ratio=round(statistics.median(push_ms[name]) / statistics.median(push_ms[against]), 4),
                              lock_at_the_end=legs[name].read_input_afc(0))), flush=True)
for rx in legs.values():
    rx.close()
