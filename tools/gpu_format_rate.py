#!/usr/bin/env python3
"""What the sample formats (cfg.input_format, cfg.input_gain_q8) cost: 128 captures x 2^22 raw samples, HBM-resident, through
wmbus_batch, `--steps` timed pushes per context after `--warmup`, all legs alternating `--rounds` times in one process (DESIGN.md
section 6: one box visit, interleaved).  Legs:

    rs-cu8 rs-cs8 rs-cs16 rs-cf32      2.048 MS/s in that format through the resampler (the wide formats 6 bits down, gain 64)
    parent-rs-cu8                      rs-cu8 on another build of the library (--parent-lib: the parent commit's), the A/B of the cu8 path
    native                             cu8 at 1.6 MS/s, no K0 stage at all
    cv-cu8 cv-cs8 cv-cs16 cv-cf32      1.6 MS/s in that format through the conversion kernel (cu8: gain 257 / 256, which switches it on)
    rs25-cs16 (not in the default list) cs16 at 2.5 MS/s through the resampler
    LEG+shift                          any leg but native / parent-*: the same with cfg.input_shift_hz = --shift-hz, i.e. the rotating
                                       instantiation of its kernel (cv-cu8+shift: the shift alone switches the conversion kernel on, gain x 1).
                                       The captures are NOT mixed up to match, so nothing decodes behind K0: read a +shift leg's K0 kernel
                                       time below, not its job rate

Prints one JSON line per leg and round: raw input Msamples/s, and the clipped share.  `--copy-bandwidth` also times a device-to-device
copy of 1 GiB (hipMemcpyAsync; read + write bytes per second), the yardstick for the conversion kernel.  Needs a GPU.

Kernel times: `rocprofv3 --kernel-trace --stats -d DIR -o k0 --output-format csv -- python tools/gpu_format_rate.py --rounds 1
--steps 5`, rows k0_resample*, k0_convert* and k1_demod2 of the kernel statistics."""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
wm = importlib.import_module("rtl-wmbus_amd")
import format_ref as FR  # noqa: E402  (the embeddings; the bytes are not checked here)

ALL = "rs-cu8,parent-rs-cu8,rs-cs8,rs-cs16,rs-cf32,native,cv-cu8,cv-cs8,cv-cs16,cv-cf32"
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--legs", default=ALL)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--distinct", type=int, default=8, help="distinct synthetic captures (the others repeat them)")
ap.add_argument("--log2-samples", type=int, default=22)
ap.add_argument("--parent-lib", default=None, help="libwmbus_hip.so of the parent commit (leg parent-rs-cu8; skipped without it)")
ap.add_argument("--shift-hz", type=int, default=200000, help="cfg.input_shift_hz of the +shift legs")
ap.add_argument("--copy-bandwidth", action="store_true")
a = ap.parse_args()
if wm.device_count() < 1:
    sys.exit("gpu_format_rate.py: no HIP device")


def second_copy(lib_path):
    """The package again, bound to another build of the library (with the __init__.py of that build where one lies next to the
    library: a build of another commit may miss exports this mirror binds, or lay wmbus_cfg out differently)."""
    os.environ["WMBUS_HIP_LIB"] = lib_path
    mirror = os.path.join(os.path.dirname(os.path.abspath(lib_path)), "__init__.py")      # that build's own ctypes mirror, if it lies beside it
    spec = importlib.util.spec_from_file_location("wm_parent", mirror if os.path.exists(mirror) else os.path.join(ROOT, "rtl-wmbus_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    del os.environ["WMBUS_HIP_LIB"]
    return mod


n = 1 << a.log2_samples
FMT = {"cu8": FR.CU8, "cs8": FR.CS8, "cs16": FR.CS16, "cf32": FR.CF32}
synth = {}


def capture(fs_khz, s, fmt):
    key = (fs_khz, s)
    if key not in synth:
        synth[key] = wm.synth_capture(seed=0xC0FFEE + s, n_samples=n, fs_khz=fs_khz, kinds=7, frames_per_s=20.0)[0]
    raw = FR.embed(synth[key], fmt)
    if fmt in (FR.CS16, FR.CF32):                            # a weak wide capture: 6 bits down, brought back by the gain
        raw = FR.raw_bytes(raw.view("<i2") >> 6, fmt) if fmt == FR.CS16 else FR.raw_bytes(raw.view("<f4") / np.float32(64), fmt)
    return raw


batches, meta = {}, {}
for leg in a.legs.split(","):
    mod, kw, fs = wm, {}, 1600
    shifted = leg.endswith("+shift")
    leg_name, leg = leg, leg[:-len("+shift")] if shifted else leg
    if leg == "native":
        fmt = FR.CU8
    else:
        kind, name = leg.rsplit("-", 1)
        fmt = FMT[name]
        if kind.endswith("rs"):
            fs, kw = 2048, dict(input_rate_hz=2048000)
        elif kind == "rs25":
            fs, kw = 2500, dict(input_rate_hz=2500000)
        if kind == "parent-rs":
            if not a.parent_lib:
                continue
            mod = second_copy(a.parent_lib)
        else:
            gain = 64 * 256 if fmt in (FR.CS16, FR.CF32) else 257 if leg == "cv-cu8" and not shifted else 0
            kw.update(input_format=fmt, input_gain_q8=gain)
            if shifted:
                kw.update(input_shift_hz=a.shift_hz)
    bps = FR.BPS[fmt]
    b = mod.Batch(n_streams=a.streams, max_push_bytes=bps * n, **kw)
    for s in range(a.streams):
        b.stage(s, capture(fs, s % a.distinct, fmt))
    b.run_resident(bps * n, a.warmup)
    leg = leg_name
    batches[leg], meta[leg] = b, dict(fmt=FR.NAMES[fmt], bytes_per_sample=bps, fs_khz=fs, **{k: int(v) for k, v in kw.items()})
for r in range(a.rounds):
    for leg, b in batches.items():
        clip = [0, 0]

        def on_push(first, k, lines, tm, clip=clip):
            clip[0] += tm.get("input_clipped", 0); clip[1] += tm.get("input_bytes_out", 0)
        st = b.run_resident(meta[leg]["bytes_per_sample"] * n, a.steps, on_push=None if leg.startswith("parent") else on_push, want_lines=False)
        print(json.dumps(dict(leg=leg, round=r, **meta[leg], streams=a.streams, raw_samples_per_stream=n, contexts=len(b.contexts), steps=a.steps,
                              seconds=round(st["seconds"], 4), lines=st["lines"], raw_msamples_per_s=round(st["samples"] / st["seconds"] / 1e6, 1),
                              clipped_share=(clip[0] / clip[1] if clip[1] else None))), flush=True)
for b in batches.values():
    b.close()

if a.copy_bandwidth:
    import ctypes
    import time
    hip = ctypes.CDLL("libamdhip64.so")
    nbytes, reps = 1 << 30, 10
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)) == 0 and hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)) == 0
    for k in range(3 + reps):
        if k == 3:
            hip.hipDeviceSynchronize(); t0 = time.perf_counter()
        assert hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, None) == 0       # 3: hipMemcpyDeviceToDevice
    hip.hipDeviceSynchronize()
    dt = time.perf_counter() - t0
    hip.hipFree(src); hip.hipFree(dst)
    print(json.dumps(dict(leg="copy", gib=1, reps=reps, read_plus_write_gb_per_s=round(2 * reps * nbytes / dt / 1e9, 1))), flush=True)
