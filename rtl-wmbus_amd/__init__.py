"""rtl-wmbus_amd -- MI355X-native back end for the rtl-wmbus cu8 -> datagram hot path.

Thin ctypes mirror of the C ABI in include/wmbus_hip.h (libwmbus_hip.so: hand-written HIP kernels
for gfx950 + host packet decoders).  The directory name contains a hyphen, so import it with

    import importlib; wm = importlib.import_module("rtl-wmbus_amd")

There is no CPU fallback: opening a receiver without a HIP device raises WmbusError.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WMBUS_HIP_LIB") or os.path.join(HERE, "libwmbus_hip.so")   # override: A/B of two builds
SYNTH_PATH = os.path.join(HERE, "libwmbus_synth.so")
CLI_PATH = os.path.join(HERE, "rtl_wmbus_hip")

CHAIN_T1C1, CHAIN_S1 = 0, 1
ALGO_RLA, ALGO_T2A = 0, 1
BLOCK_BYTES = 4096


class WmbusError(RuntimeError):
    pass


def build(force=False):
    """Compile every native target for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-s", "-C", HERE, "clean"], check=True)
    subprocess.run(["make", "-s", "-C", HERE], check=True)


MAX_CHANNELS = 8                                    # WMBUS_MAX_CHANNELS


class Cfg(ctypes.Structure):
    _fields_ = [("decimation", ctypes.c_uint), ("simultaneous", ctypes.c_int), ("accurate_atan", ctypes.c_int),
                ("remove_dc", ctypes.c_int), ("t1c1_enabled", ctypes.c_int), ("s1_enabled", ctypes.c_int),
                ("rla_enabled", ctypes.c_int), ("time2_enabled", ctypes.c_int), ("show_algorithm", ctypes.c_int),
                ("fixed_timestamp", ctypes.c_int), ("n_streams", ctypes.c_uint), ("device", ctypes.c_int),
                ("max_push_bytes", ctypes.c_size_t), ("seg_len", ctypes.c_uint), ("rla_seg_len", ctypes.c_uint),
                ("warmup_t1c1", ctypes.c_uint),
                ("warmup_s1", ctypes.c_uint), ("rla_lookback", ctypes.c_uint), ("host_threads", ctypes.c_uint),
                ("keep_taps", ctypes.c_int), ("prefilter", ctypes.c_int), ("atan_mode", ctypes.c_int), ("spill_words", ctypes.c_uint), ("dedup_twins", ctypes.c_int), ("only_crc_ok", ctypes.c_int),
                ("s1_rescue", ctypes.c_uint), ("input_windows", ctypes.c_uint), ("line_quality", ctypes.c_uint), ("tolerance_mode", ctypes.c_int),
                # tuning and test knobs (0 = default), wmbus_hip.h
                ("crc_repair", ctypes.c_uint), ("rounds_on_host", ctypes.c_uint), ("channel_activity", ctypes.c_uint), ("channel_activity_ratio_q8", ctypes.c_uint),
                ("rssi_full", ctypes.c_uint), ("rssi_dense_pm", ctypes.c_uint), ("line_power", ctypes.c_uint), ("bursts_to_host", ctypes.c_uint),
                ("input_spectrum_age", ctypes.c_uint), ("input_channel_afc_hz", ctypes.c_uint * MAX_CHANNELS),
                ("burst_caps", ctypes.c_uint * 4), ("input_afc", ctypes.c_uint), ("input_afc_range_hz", ctypes.c_uint), ("k1_small_tile", ctypes.c_uint),
                ("input_spectrum", ctypes.c_uint), ("input_channels", ctypes.c_uint), ("input_channel_hz", ctypes.c_int * MAX_CHANNELS),
                ("k1_tiles_per_block", ctypes.c_uint), ("input_agc", ctypes.c_uint), ("clock_waves", ctypes.c_uint),
                ("line_levels", ctypes.c_uint),
                ("input_rate_hz", ctypes.c_uint), ("input_shift_hz", ctypes.c_int), ("input_dc", ctypes.c_uint), ("input_format", ctypes.c_uint), ("input_gain_q8", ctypes.c_uint)]


class Line(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint32), ("chain", ctypes.c_uint8), ("algo", ctypes.c_uint8),
                ("crc_ok", ctypes.c_uint8), ("pad", ctypes.c_uint8), ("sample", ctypes.c_uint64),
                ("text_off", ctypes.c_uint32), ("text_len", ctypes.c_uint32)]
    # wmbus_line.channel: the byte that was wmbus_line.pad (same offset and size; this mirror keeps the byte's old name as its storage)
    channel = property(lambda self: int(self.pad))


class Level(ctypes.Structure):
    """wmbus_level: the frequency offset and the mean absolute deviation of a line's telegram (cfg.line_levels); n = 0: not measured."""
    _fields_ = [("sync_sample", ctypes.c_uint64), ("offset_hz", ctypes.c_int32), ("dev_hz", ctypes.c_uint32), ("n", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]

    def as_dict(self):
        return dict(sync_sample=int(self.sync_sample), offset_hz=int(self.offset_hz), dev_hz=int(self.dev_hz), n=int(self.n))


class Power(ctypes.Structure):
    """wmbus_power: the signal in a line's channel, the noise floor in front of its telegram and their ratio (cfg.line_power), from the raw
    input; n_signal / n_noise = 0: not measured."""
    _fields_ = [("first_block", ctypes.c_uint64), ("signal", ctypes.c_uint32), ("noise", ctypes.c_uint32), ("ratio_q8", ctypes.c_uint32),
                ("n_signal", ctypes.c_uint16), ("n_noise", ctypes.c_uint16)]

    def as_dict(self):
        return dict(first_block=int(self.first_block), signal=int(self.signal), noise=int(self.noise), ratio_q8=int(self.ratio_q8),
                    n_signal=int(self.n_signal), n_noise=int(self.n_noise))


class Burst(ctypes.Structure):
    """wmbus_burst: one burst of energy in a pipeline row's channel (cfg.channel_activity), decoded or not."""
    _fields_ = [("first_block", ctypes.c_uint64), ("blocks", ctypes.c_uint32), ("mean", ctypes.c_uint32), ("floor", ctypes.c_uint32),
                ("stream", ctypes.c_uint32), ("channel", ctypes.c_uint8), ("chain", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 2)]

    def as_dict(self):
        return dict(first_block=int(self.first_block), blocks=int(self.blocks), mean=int(self.mean), floor=int(self.floor),
                    stream=int(self.stream), channel=int(self.channel), chain=int(self.chain))


class Repair(ctypes.Structure):
    """wmbus_repair: what CRC repair did for a line's telegram (cfg.crc_repair); all zero: clean, or no subject."""
    _fields_ = [("blocks_bad", ctypes.c_uint16), ("blocks_repaired", ctypes.c_uint16), ("chips_flipped", ctypes.c_uint16), ("pad", ctypes.c_uint16),
                ("weight", ctypes.c_uint32)]

    def as_dict(self):
        return dict(blocks_bad=int(self.blocks_bad), blocks_repaired=int(self.blocks_repaired), chips_flipped=int(self.chips_flipped), weight=int(self.weight))


class Rescue(ctypes.Structure):
    """wmbus_rescue: what S1 rescue did for a line's telegram (cfg.s1_rescue); all zero: the line is no rescue."""
    _fields_ = [("status", ctypes.c_uint16), ("pairs", ctypes.c_uint16), ("min_margin", ctypes.c_uint32), ("blocks", ctypes.c_uint16), ("pad", ctypes.c_uint16)]

    def as_dict(self):
        return dict(status=int(self.status), pairs=int(self.pairs), min_margin=int(self.min_margin), blocks=int(self.blocks))


class Quality(ctypes.Structure):
    """wmbus_quality: chip rate, jitter and eye of a line's telegram (cfg.line_quality); n = 0: not measured."""
    _fields_ = [("n", ctypes.c_uint32), ("chip_rate_chz", ctypes.c_uint32), ("jitter_ns", ctypes.c_uint32), ("hi_hz", ctypes.c_int32), ("lo_hz", ctypes.c_int32),
                ("spread_hz", ctypes.c_uint32), ("eye_hz", ctypes.c_int32), ("pad", ctypes.c_uint32)]

    def as_dict(self):
        return dict(n=int(self.n), chip_rate_chz=int(self.chip_rate_chz), jitter_ns=int(self.jitter_ns), hi_hz=int(self.hi_hz), lo_hz=int(self.lo_hz),
                    spread_hz=int(self.spread_hz), eye_hz=int(self.eye_hz))


class ChannelHit(ctypes.Structure):
    """wmbus_channel_hit: one channel of a survey (wmbus_spectrum_channels)."""
    _fields_ = [("offset_hz", ctypes.c_int32), ("ratio_q8", ctypes.c_uint32), ("floor_peak", ctypes.c_uint32), ("floor_mean", ctypes.c_uint32)]

    def as_dict(self):
        return dict(offset_hz=int(self.offset_hz), ratio_q8=int(self.ratio_q8), floor_peak=int(self.floor_peak), floor_mean=int(self.floor_mean))


SPECTRUM_BINS = 512


class Afc(ctypes.Structure):
    """wmbus_afc: the lock a capture's last push was rotated with (cfg.input_afc, Receiver.read_input_afc)."""
    _fields_ = [("shift_hz", ctypes.c_int32), ("locked", ctypes.c_uint32), ("changes", ctypes.c_uint32), ("ratio_q8", ctypes.c_uint32)]

    def as_dict(self):
        return dict(shift_hz=int(self.shift_hz), locked=int(self.locked), changes=int(self.changes), ratio_q8=int(self.ratio_q8))


class Timing(ctypes.Structure):
    _fields_ = [("demod_ms", ctypes.c_float), ("clock_ms", ctypes.c_float), ("rla_ms", ctypes.c_float),
                ("gather_ms", ctypes.c_float), ("d2h_ms", ctypes.c_float), ("gpu_total_ms", ctypes.c_float),
                ("host_decode_ms", ctypes.c_float), ("clock_reruns", ctypes.c_uint), ("rla_reruns", ctypes.c_uint),
                ("ema_retries", ctypes.c_uint), ("chips", (ctypes.c_uint64 * 2) * 2), ("bursts", ctypes.c_uint64),
                ("turn_wait_ms", ctypes.c_float), ("warnings", ctypes.c_uint), ("slow_path", ctypes.c_uint),
                ("rssi_ms", ctypes.c_float), ("rssi_mode", ctypes.c_uint), ("rssi_tiles", ctypes.c_uint),
                ("clock_round", ctypes.c_uint * 4), ("rla_round", ctypes.c_uint * 4),
                ("input_bytes_out", ctypes.c_uint64), ("input_clipped", ctypes.c_uint64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("demod_ms", "clock_ms", "rla_ms", "gather_ms", "d2h_ms", "gpu_total_ms",
                                           "host_decode_ms", "clock_reruns", "rla_reruns", "ema_retries", "bursts", "turn_wait_ms", "warnings", "slow_path",
                                           "rssi_ms", "rssi_mode", "rssi_tiles", "input_bytes_out", "input_clipped")}
        d["chips"] = [[int(self.chips[ch][al]) for al in range(2)] for ch in range(2)]      # [chain][algo]
        d["clock_round"] = [int(v) for v in self.clock_round]; d["rla_round"] = [int(v) for v in self.rla_round]
        return d


RSSI_EVERY_SAMPLE, RSSI_ON_DEMAND, RSSI_PAUSED, RSSI_FELL_BACK = 0, 1, 2, 3            # wmbus_timing.rssi_mode
FMT_CU8, FMT_CS8, FMT_CS16, FMT_CF32 = 0, 1, 2, 3                                      # wmbus_cfg.input_format
FMT_BYTES_PER_SAMPLE = {FMT_CU8: 2, FMT_CS8: 2, FMT_CS16: 4, FMT_CF32: 8}


FILL_FN = ctypes.CFUNCTYPE(ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t)
LINES_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(Line), ctypes.c_size_t, ctypes.c_void_p,
                            ctypes.POINTER(Timing))


class BatchIo(ctypes.Structure):
    _fields_ = [("fill", FILL_FN), ("lines", LINES_FN), ("user", ctypes.c_void_p), ("resident_bytes", ctypes.c_size_t), ("passes", ctypes.c_uint),
                ("self_staged", ctypes.c_uint)]


class BatchStats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_uint64), ("lines", ctypes.c_uint64), ("seconds", ctypes.c_double), ("pushes", ctypes.c_uint),
                ("warnings", ctypes.c_uint)]


EXPORTS = ["wmbus_batch_plan", "wmbus_batch_open", "wmbus_batch_close", "wmbus_batch_last_error", "wmbus_batch_contexts", "wmbus_batch_context", "wmbus_batch_stage",
           "wmbus_batch_device_input", "wmbus_batch_run", "wmbus_batch_lane_stats",
           "wmbus_runtime_init", "wmbus_default_cfg", "wmbus_open", "wmbus_close", "wmbus_last_error", "wmbus_stage", "wmbus_device_input",
           "wmbus_process", "wmbus_collect", "wmbus_lines", "wmbus_lines_text", "wmbus_get_timing", "wmbus_read_tap",
           "wmbus_read_chips", "wmbus_device_count", "wmbus_selftest_math", "wmbus_selftest_fir", "wmbus_selftest_udiv", "wmbus_alloc_pinned", "wmbus_free_pinned",
           "wmbus_debug_replay_decode", "wmbus_resampler_design", "wmbus_read_resampled", "wmbus_resampler_launches", "wmbus_shift_design", "wmbus_read_input_dc", "wmbus_read_input_gain",
           "wmbus_line_levels", "wmbus_batch_line_levels", "wmbus_read_spectrum", "wmbus_spectrum_channels", "wmbus_read_input_afc",
           "wmbus_line_power", "wmbus_batch_line_power", "wmbus_read_waterfall", "wmbus_read_channel_power", "wmbus_line_power_rule", "wmbus_line_power_block",
           "wmbus_activity", "wmbus_activity_progress", "wmbus_batch_activity", "wmbus_activity_rule", "wmbus_activity_match",
           "wmbus_line_repairs", "wmbus_batch_line_repairs", "wmbus_line_quality", "wmbus_batch_line_quality",
           "wmbus_line_rescues", "wmbus_batch_line_rescues", "wmbus_rescue_stats"]

_lib = None


def lib():
    """Load libwmbus_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WmbusError(f"{LIB_PATH} is missing: run __graft_entry__.build() / make -C rtl-wmbus_amd")
        L = ctypes.CDLL(LIB_PATH)
        L.wmbus_runtime_init()           # before the first HIP call of the process (the hardware-queue default, see wmbus_hip.h)
        vp, u, sz = ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t
        L.wmbus_default_cfg.argtypes = [ctypes.POINTER(Cfg)]
        L.wmbus_open.argtypes = [ctypes.POINTER(Cfg), ctypes.POINTER(vp)]
        L.wmbus_close.argtypes = [vp]
        L.wmbus_last_error.argtypes = [vp]; L.wmbus_last_error.restype = ctypes.c_char_p
        L.wmbus_stage.argtypes = [vp, u, vp, sz]
        L.wmbus_device_input.argtypes = [vp, u]; L.wmbus_device_input.restype = vp
        L.wmbus_process.argtypes = [vp, sz]
        L.wmbus_collect.argtypes = [vp]
        L.wmbus_lines.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Line))]; L.wmbus_lines.restype = sz
        L.wmbus_lines_text.argtypes = [vp, ctypes.POINTER(sz)]; L.wmbus_lines_text.restype = vp
        L.wmbus_line_levels.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Level))]; L.wmbus_line_levels.restype = sz
        L.wmbus_batch_line_levels.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Level))]; L.wmbus_batch_line_levels.restype = sz
        L.wmbus_get_timing.argtypes = [vp, ctypes.POINTER(Timing)]
        L.wmbus_read_tap.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, u, vp, sz]; L.wmbus_read_tap.restype = ctypes.c_long
        L.wmbus_read_chips.argtypes = [vp, ctypes.c_int, ctypes.c_int, u, vp, vp, sz]; L.wmbus_read_chips.restype = ctypes.c_long
        L.wmbus_device_count.restype = ctypes.c_int
        L.wmbus_resampler_design.argtypes = [u, u, ctypes.POINTER(u), ctypes.POINTER(u), ctypes.POINTER(u), vp, sz]
        L.wmbus_shift_design.argtypes = [u, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), vp, sz]
        L.wmbus_read_resampled.argtypes = [vp, u, vp, sz]; L.wmbus_read_resampled.restype = ctypes.c_long
        L.wmbus_read_input_dc.argtypes = [vp, u, vp, sz]; L.wmbus_read_input_dc.restype = ctypes.c_long
        L.wmbus_read_input_gain.argtypes = [vp, u, vp, sz]; L.wmbus_read_input_gain.restype = ctypes.c_long
        L.wmbus_read_spectrum.argtypes = [vp, u, vp, vp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]; L.wmbus_read_spectrum.restype = ctypes.c_long
        L.wmbus_spectrum_channels.argtypes = [u, vp, vp, ctypes.c_uint64, u, u, u, ctypes.POINTER(ChannelHit), u]
        L.wmbus_read_input_afc.argtypes = [vp, u, ctypes.POINTER(Afc)]; L.wmbus_read_input_afc.restype = ctypes.c_long
        L.wmbus_line_power.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Power))]; L.wmbus_line_power.restype = sz
        L.wmbus_batch_line_power.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Power))]; L.wmbus_batch_line_power.restype = sz
        L.wmbus_read_waterfall.argtypes = [vp, u, vp, ctypes.POINTER(ctypes.c_uint64), sz]; L.wmbus_read_waterfall.restype = ctypes.c_long
        L.wmbus_read_channel_power.argtypes = [vp, ctypes.c_int, u, vp, ctypes.POINTER(ctypes.c_uint64), sz]; L.wmbus_read_channel_power.restype = ctypes.c_long
        L.wmbus_line_power_rule.argtypes = [vp, ctypes.c_uint64, sz, ctypes.c_uint64, ctypes.c_uint64, u, ctypes.POINTER(Power)]
        L.wmbus_line_power_block.argtypes = [u, u, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.wmbus_activity.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Burst))]; L.wmbus_activity.restype = sz
        L.wmbus_activity_progress.argtypes = [vp]; L.wmbus_activity_progress.restype = ctypes.c_uint64
        L.wmbus_batch_activity.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Burst))]; L.wmbus_batch_activity.restype = sz
        L.wmbus_activity_rule.argtypes = [vp, sz, u, u, ctypes.POINTER(Burst), sz]; L.wmbus_activity_rule.restype = ctypes.c_long
        L.wmbus_activity_match.argtypes = [ctypes.POINTER(Burst), sz, u, u, ctypes.c_int, ctypes.c_uint64]; L.wmbus_activity_match.restype = ctypes.c_long
        L.wmbus_line_repairs.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Repair))]; L.wmbus_line_repairs.restype = sz
        L.wmbus_batch_line_repairs.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Repair))]; L.wmbus_batch_line_repairs.restype = sz
        L.wmbus_line_quality.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Quality))]; L.wmbus_line_quality.restype = sz
        L.wmbus_batch_line_quality.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Quality))]; L.wmbus_batch_line_quality.restype = sz
        L.wmbus_line_rescues.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(Rescue))]; L.wmbus_line_rescues.restype = sz
        L.wmbus_batch_line_rescues.argtypes = [vp, u, ctypes.POINTER(ctypes.POINTER(Rescue))]; L.wmbus_batch_line_rescues.restype = sz
        L.wmbus_rescue_stats.argtypes = [vp, ctypes.POINTER(u), ctypes.POINTER(u)]
        L.wmbus_resampler_launches.argtypes = [vp]; L.wmbus_resampler_launches.restype = ctypes.c_ulonglong
        L.wmbus_alloc_pinned.argtypes = [sz]; L.wmbus_alloc_pinned.restype = vp
        L.wmbus_free_pinned.argtypes = [vp]
        L.wmbus_selftest_math.argtypes = [ctypes.c_int] + [vp] * 6 + [sz]
        L.wmbus_selftest_fir.argtypes = [ctypes.c_int, vp, vp, sz]
        if hasattr(L, "wmbus_selftest_udiv"):               # an A/B against an earlier build (WMBUS_HIP_LIB) still loads
            L.wmbus_selftest_udiv.argtypes = [ctypes.c_int, vp, ctypes.POINTER(ctypes.c_ulonglong)]; L.wmbus_selftest_udiv.restype = ctypes.c_longlong
        L.wmbus_debug_replay_decode.argtypes = [vp, u, ctypes.POINTER(ctypes.c_double)]; L.wmbus_debug_replay_decode.restype = ctypes.c_long
        L.wmbus_batch_open.argtypes = [ctypes.POINTER(Cfg), u, ctypes.POINTER(vp)]
        L.wmbus_batch_plan.argtypes = [ctypes.POINTER(Cfg), u, ctypes.POINTER(u), u]; L.wmbus_batch_plan.restype = u
        L.wmbus_batch_close.argtypes = [vp]
        L.wmbus_batch_last_error.argtypes = [vp]; L.wmbus_batch_last_error.restype = ctypes.c_char_p
        L.wmbus_batch_contexts.argtypes = [vp]; L.wmbus_batch_contexts.restype = u
        if hasattr(L, "wmbus_batch_lane_stats"):            # an A/B against a build from before lanes (WMBUS_HIP_LIB) still loads
            L.wmbus_batch_lane_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
            L.wmbus_batch_lane_stats.restype = ctypes.c_int
        L.wmbus_batch_context.argtypes = [vp, u, ctypes.POINTER(u), ctypes.POINTER(u)]; L.wmbus_batch_context.restype = vp
        L.wmbus_batch_stage.argtypes = [vp, u, vp, sz]
        L.wmbus_batch_device_input.argtypes = [vp, u]; L.wmbus_batch_device_input.restype = vp
        L.wmbus_batch_run.argtypes = [vp, ctypes.POINTER(BatchIo), ctypes.POINTER(BatchStats)]
        _lib = L
    return _lib


def device_count():
    return int(lib().wmbus_device_count())


def resampler_design(in_hz, out_hz):
    """wmbus_resampler_design (host only): (L, M, T, taps int16 [L, T]) of the exact integer resampler behind
    Receiver(input_rate_hz=...); raises WmbusError for a ratio the library does not take."""
    L_, M_, T_ = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_uint()
    rc = lib().wmbus_resampler_design(int(in_hz), int(out_hz), ctypes.byref(L_), ctypes.byref(M_), ctypes.byref(T_), None, 0)
    if rc:
        raise WmbusError(f"wmbus_resampler_design({in_hz}, {out_hz}) failed: {rc}")
    taps = np.zeros((L_.value, T_.value), np.int16)
    rc = lib().wmbus_resampler_design(int(in_hz), int(out_hz), ctypes.byref(L_), ctypes.byref(M_), ctypes.byref(T_), taps.ctypes.data, taps.size)
    if rc:
        raise WmbusError(f"wmbus_resampler_design({in_hz}, {out_hz}) failed: {rc}")
    return L_.value, M_.value, T_.value, taps


def shift_design(in_hz, shift_hz):
    """wmbus_shift_design (host only): (step, table int16 [1024, 2] of {c, s}) of the exact integer frequency shift behind
    Receiver(input_shift_hz=...); raises WmbusError for a shift beyond half the input rate."""
    step = ctypes.c_uint32()
    table = np.zeros((1024, 2), np.int16)
    rc = lib().wmbus_shift_design(int(in_hz), int(shift_hz), ctypes.byref(step), table.ctypes.data, table.size)
    if rc:
        raise WmbusError(f"wmbus_shift_design({in_hz}, {shift_hz}) failed: {rc}")
    return step.value, table


def spectrum_channels(in_hz, total, peak, blocks, width_hz=0, min_ratio_q8=0, rel=0, cap=64):
    """wmbus_spectrum_channels (host only): the channels of a survey -- (sum, peak, blocks) as Receiver.read_spectrum returns them -- as a
    list of dicts offset_hz (the value input_shift_hz / input_channel_hz want), ratio_q8, floor_peak, floor_mean, strongest first.  0 takes
    the library's default (width 200 kHz, ratio x 4, rel 8); raises WmbusError where the library refuses."""
    total = np.ascontiguousarray(total, np.uint64); peak = np.ascontiguousarray(peak, np.uint32)
    assert total.size == SPECTRUM_BINS and peak.size == SPECTRUM_BINS
    out = (ChannelHit * max(1, int(cap)))()
    n = lib().wmbus_spectrum_channels(int(in_hz), total.ctypes.data, peak.ctypes.data, int(blocks), int(width_hz), int(min_ratio_q8), int(rel), out, int(cap))
    if n < 0:
        raise WmbusError(f"wmbus_spectrum_channels failed: {n}")
    return [out[i].as_dict() for i in range(n)]


def line_power_rule(p, first_block, ka, ke, in_hz):
    """wmbus_line_power_rule (host only): the power record of a line whose access code lies in level block ka and whose last chip in ke,
    from p = P of level blocks first_block ... as Receiver.read_channel_power returns it; a dict of the record's fields."""
    p = np.ascontiguousarray(p, np.uint32)
    out = Power()
    rc = lib().wmbus_line_power_rule(p.ctypes.data if p.size else None, int(first_block), p.size, int(ka), int(ke), int(in_hz), ctypes.byref(out))
    if rc:
        raise WmbusError(f"wmbus_line_power_rule failed: {rc}")
    return out.as_dict()


def line_power_block(sample, decimation=2, input_rate_hz=0):
    """wmbus_line_power_block (host only): the level block of the raw input that decimated sample `sample` stands for."""
    out = ctypes.c_uint64()
    rc = lib().wmbus_line_power_block(int(decimation), int(input_rate_hz), int(sample), ctypes.byref(out))
    if rc:
        raise WmbusError(f"wmbus_line_power_block failed: {rc}")
    return int(out.value)


def activity_rule(p, in_hz, ratio_q8=0):
    """wmbus_activity_rule (host only): the bursts of one row's whole timeline p = P of level blocks 0 ... (CHANNEL ACTIVITY); a list of
    dicts like Receiver.activity()'s, stream, channel and chain 0."""
    p = np.ascontiguousarray(p, np.uint32)
    cap = p.size // 3 + 2
    out = (Burst * cap)()
    n = lib().wmbus_activity_rule(p.ctypes.data if p.size else None, p.size, int(in_hz), int(ratio_q8), out, cap)
    if n < 0:
        raise WmbusError(f"wmbus_activity_rule failed: {n}")
    return [out[i].as_dict() for i in range(n)]


def activity_match(records, stream, channel, chain, ka):
    """wmbus_activity_match (host only): the index in `records` (dicts as Receiver.activity() returns them) of the burst of row (stream,
    channel, chain) that a line with access-code level block ka belongs to, or -1."""
    arr = (Burst * max(1, len(records)))()
    for i, r in enumerate(records):
        arr[i] = Burst(r["first_block"], r["blocks"], r["mean"], r["floor"], r["stream"], r["channel"], r["chain"])
    return int(lib().wmbus_activity_match(arr, len(records), int(stream), int(channel), int(chain), int(ka)))


def pinned_array(nbytes):
    """uint8 numpy array over page-locked host memory (kept alive by the array's base object)."""
    p = lib().wmbus_alloc_pinned(nbytes)
    if not p:
        raise WmbusError("wmbus_alloc_pinned failed")

    class _Owner:
        def __init__(self, ptr): self.ptr = ptr
        def __del__(self): lib().wmbus_free_pinned(self.ptr)
    buf = (ctypes.c_uint8 * nbytes).from_address(p)
    buf._owner = _Owner(p)
    return np.frombuffer(buf, np.uint8)


def selftest_math(a, b, device=0):
    """Device sqrt / divide / atan2f / discriminator of wm_exact.h on float32 arrays a, b."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    outs = [np.empty_like(a) for _ in range(4)]
    rc = lib().wmbus_selftest_math(device, a.ctypes.data, b.ctypes.data, *[o.ctypes.data for o in outs], a.size)
    if rc:
        raise WmbusError(f"selftest_math failed: {rc}")
    return dict(sqrt=outs[0], div=outs[1], atan2=outs[2], disc=outs[3])


def selftest_fir(x, device=0):
    """The demodulation kernel's 11-tap and 46-tap low-pass filters on the device: x = 48 samples of history + n inputs
    (n a multiple of 4, <= 976); returns (y11[n], y46[n])."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.size - 48
    out = np.empty(2 * n, np.float32)
    rc = lib().wmbus_selftest_fir(device, x.ctypes.data, out.ctypes.data, n)
    if rc:
        raise WmbusError(f"selftest_fir failed: {rc}")
    return out[:n], out[n:]


def selftest_udiv(device=0):
    """The run-length kernel's integer divisions over their domain, compared on the device with the compiler's division:
    (wrong quotients, [(dividend, divisor)] of the first 16 of them, cases looked at)."""
    first = np.zeros(32, np.uint32)
    cases = ctypes.c_ulonglong(0)
    wrong = lib().wmbus_selftest_udiv(device, first.ctypes.data, ctypes.byref(cases))
    if wrong < 0:
        raise WmbusError(f"selftest_udiv failed: {wrong}")
    return int(wrong), [tuple(int(v) for v in first[2 * i:2 * i + 2]) for i in range(min(16, int(wrong)))], int(cases.value)


def _make_cfg(n_streams=1, max_push_bytes=4 << 20, decimation=2, simultaneous=False, accurate_atan=True,
              remove_dc=False, t1c1=True, s1=True, rla=True, time2=True, show_algorithm=True, device=0,
              seg_len=0, rla_seg_len=0, warmup_t1c1=0, warmup_s1=0, rla_lookback=0, host_threads=0, fixed_timestamp=True,
              prefilter=0, atan_mode=0, keep_taps=True, spill_words=0, input_windows=1, dedup_twins=False, only_crc_ok=False, tolerance_mode=0,
              rounds_on_host=False, rssi_full=False, rssi_dense_pm=0, bursts_to_host=False, burst_caps=None, k1_small_tile=False, k1_tiles_per_block=0, clock_waves=0,
              input_rate_hz=0, input_format=0, input_gain_q8=0, input_shift_hz=0, input_dc=0, input_agc=0, line_levels=0,
              input_channel_hz=None, input_spectrum=0, input_afc=0, input_afc_range_hz=0, input_spectrum_age=0, input_channel_afc_hz=None, line_power=0,
              channel_activity=0, channel_activity_ratio_q8=0, crc_repair=0, line_quality=0, s1_rescue=0):
    c = Cfg()
    lib().wmbus_default_cfg(ctypes.byref(c))
    # test campaigns (tests/README.md): the whole GPU suite once with every hand-off failure finished by the host-driven path,
    # once with every burst through the host packet decoders -- defaults of THIS wrapper, the library reads no environment
    rounds_on_host = rounds_on_host or os.environ.get("WMBUS_TEST_ROUNDS_ON_HOST") == "1"
    bursts_to_host = bursts_to_host or (os.environ.get("WMBUS_TEST_BURSTS_TO_HOST") == "1" and not crc_repair and not line_quality and not s1_rescue)      # crc_repair, line_quality and s1_rescue refuse it: that campaign's default gives way
    c.decimation, c.simultaneous, c.accurate_atan, c.remove_dc = decimation, int(simultaneous), int(accurate_atan), int(remove_dc)
    c.t1c1_enabled, c.s1_enabled, c.rla_enabled, c.time2_enabled = int(t1c1), int(s1), int(rla), int(time2)
    c.show_algorithm, c.fixed_timestamp = int(show_algorithm), int(fixed_timestamp)
    c.n_streams, c.device, c.max_push_bytes = n_streams, device, max_push_bytes
    c.seg_len, c.rla_seg_len, c.warmup_t1c1, c.warmup_s1 = seg_len, rla_seg_len, warmup_t1c1, warmup_s1
    c.rla_lookback, c.host_threads = rla_lookback, host_threads
    c.keep_taps, c.prefilter, c.atan_mode, c.spill_words, c.input_windows = int(keep_taps), prefilter, atan_mode, spill_words, input_windows
    c.dedup_twins, c.only_crc_ok, c.tolerance_mode = int(dedup_twins), int(only_crc_ok), int(tolerance_mode)
    c.rounds_on_host, c.rssi_full, c.rssi_dense_pm, c.bursts_to_host, c.k1_small_tile = int(rounds_on_host), int(rssi_full), int(rssi_dense_pm), int(bursts_to_host), int(k1_small_tile)
    c.k1_tiles_per_block = int(k1_tiles_per_block)
    c.clock_waves = int(clock_waves)
    c.input_rate_hz = int(input_rate_hz)     # 0: the input is at decimation x 800 kHz; else the library resamples it on the GPU
    # raw sample format (FMT_*) and linear gain in Q8 (0: x 1); stage / process / max_push_bytes then count RAW bytes
    c.input_format, c.input_gain_q8 = int(input_format), int(input_gain_q8)
    c.input_shift_hz = int(input_shift_hz)   # signed Hz from the capture's centre to the channel (0: the capture is centred on it)
    c.input_dc = int(input_dc)               # 0: off; R = 1 ... 12: the I/Q DC blocker, time constant 2^R x 512 input samples
    c.input_agc = int(input_agc)             # 0: off; 1: the gain of every level block of 512 input samples from its own peak (not with input_gain_q8)
    c.input_spectrum = int(input_spectrum)   # 1: the channel survey -- a max-hold spectrum of every capture: Receiver.read_spectrum(), spectrum_channels()
    # 1: automatic frequency correction -- every capture locked to its own transmitter within input_shift_hz +- range (0: 64000 Hz),
    # found from the capture's survey and applied within the same push: Receiver.read_input_afc()
    c.input_afc, c.input_afc_range_hz = int(input_afc), int(input_afc_range_hz)
    # A = 1 ... 31: the survey forgets -- it holds the last two epochs of 2^A level blocks (2^A x 512 input samples); AFC locks on that view
    c.input_spectrum_age = int(input_spectrum_age)
    # a lock per channel of input_channel_hz: the AFC range of every channel in Hz, 0: that channel is fixed.  Entries beyond the
    # library's limit are dropped here; one beyond the channel list is passed on, so that wmbus_open refuses it with its message
    for i, r in enumerate(list(input_channel_afc_hz if input_channel_afc_hz is not None else ())[:MAX_CHANNELS]):
        c.input_channel_afc_hz[i] = int(r)
    c.channel_activity = int(channel_activity)                      # 1: a record per burst of energy in every row's channel, decoded or not: Receiver.activity()
    c.channel_activity_ratio_q8 = int(channel_activity_ratio_q8)    # its threshold over the floor in Q8 (0: 1024)
    c.crc_repair = int(crc_repair)           # 1: time2 telegrams that fail a block CRC are repaired on the GPU: Receiver.line_repairs(), Batch sinks
    c.s1_rescue = int(s1_rescue)             # 1: S1 telegrams of the time2 framer lost to a Manchester violation are decoded on the GPU from soft pairs: Receiver.line_rescues(), rescue_stats(), Batch sinks
    c.line_quality = int(line_quality)       # 1: a quality record (chip rate, jitter, eye) per line, measured on the GPU: Receiver.line_quality(), Batch sinks
    c.line_power = int(line_power)           # 1: a power record (signal, noise floor, ratio) per line from the raw input: Receiver.line_power(), read_waterfall(), read_channel_power()
    c.line_levels = int(line_levels)         # 1: a level record (frequency offset, deviation) per line: Receiver.line_levels(), Batch sinks
    # several channels of one wideband capture: signed Hz from the capture's centre to each channel (as input_shift_hz, which stays 0);
    # more entries than the library takes are passed on as a count, so that wmbus_open refuses them with its message
    hz = [int(f) for f in (input_channel_hz if input_channel_hz is not None else ())]
    c.input_channels = len(hz)
    for i, f in enumerate(hz[:MAX_CHANNELS]):
        c.input_channel_hz[i] = f
    for i, v in enumerate(burst_caps or ()):
        c.burst_caps[i] = int(v)
    return c


def batch_plan(n_streams, contexts=0, tolerance_mode=0):
    """Captures per context of a wmbus_batch of `n_streams` (no device needed)."""
    c = _make_cfg(n_streams=n_streams, tolerance_mode=tolerance_mode)
    out = (ctypes.c_uint * max(1, n_streams))()
    n = lib().wmbus_batch_plan(ctypes.byref(c), contexts, out, max(1, n_streams))
    return [int(out[i]) for i in range(n)]


class Batch:
    """wmbus_batch_*: `n_streams` captures on one device, split over several receiver contexts that the LIBRARY drives
    (include/wmbus_hip.h).  Keyword arguments as for Receiver; `contexts` = 0 takes the library's default split."""

    def __init__(self, n_streams, contexts=0, **kw):
        L = lib()
        kw.setdefault("keep_taps", False)                   # the product's configuration (the CLI's): no debug views, RSSI on demand
        self.cfg = _make_cfg(n_streams=n_streams, **kw)
        self.n_streams = n_streams
        self._h = ctypes.c_void_p()
        rc = L.wmbus_batch_open(ctypes.byref(self.cfg), contexts, ctypes.byref(self._h))
        if rc:
            msg = L.wmbus_batch_last_error(self._h).decode() if self._h else "allocation failed"
            L.wmbus_batch_close(self._h)
            self._h = None
            raise WmbusError(f"wmbus_batch_open failed ({rc}): {msg}")
        self.bursts = {}                                    # channel_activity: first stream of a context -> every burst its pushes delivered
        self.contexts = []                                  # (Receiver view, first stream, streams)
        for i in range(L.wmbus_batch_contexts(self._h)):
            f, n = ctypes.c_uint(), ctypes.c_uint()
            h = L.wmbus_batch_context(self._h, i, ctypes.byref(f), ctypes.byref(n))
            self.contexts.append((Receiver._view(h, n.value, self.cfg.input_channels), f.value, n.value))

    def close(self):
        if self._h:
            lib().wmbus_batch_close(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise WmbusError(f"error {rc}: {lib().wmbus_batch_last_error(self._h).decode()}")

    def stage(self, stream, cu8):
        cu8 = np.ascontiguousarray(cu8, dtype=np.uint8)
        self._chk(lib().wmbus_batch_stage(self._h, stream, cu8.ctypes.data, cu8.size))

    def lane_stats(self):
        """wmbus_batch_lane_stats: the batch's lanes (contexts that share a hardware queue are driven as one lane, two at most) and the
        kernel launches of the last run that carried two contexts (`paired`) or one (`single`)."""
        lanes, paired, single = ctypes.c_uint(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
        self._chk(lib().wmbus_batch_lane_stats(self._h, ctypes.byref(lanes), ctypes.byref(paired), ctypes.byref(single)))
        return dict(lanes=lanes.value, paired=paired.value, single=single.value)

    def run_resident(self, nbytes, passes, on_push=None, want_lines=True):
        """Every context makes `passes` pushes of the `nbytes` staged per stream.  on_push(first_stream, n_streams,
        [line dicts] (None unless want_lines), timing dict) is called per context push if given.  Returns the stats."""
        return self._run(BatchIo(FILL_FN(), self._sink(on_push, want_lines), None, nbytes, passes, 0))

    def run_from(self, fill, on_push=None, self_staged=False, want_lines=True):
        """Host-sourced run (input_windows=2): fill(first_stream, n_streams, slab) -> bytes per stream, where slab is a
        uint8 array [n_streams, max_push_bytes] over the library's page-locked staging memory (None with self_staged:
        the callback then stages from pinned memory of its own with Batch.stage); 0 ends that group."""
        def c_fill(user, first, n, slab, pitch, cap_):
            a = None
            if slab:
                a = np.ctypeslib.as_array(ctypes.cast(slab, ctypes.POINTER(ctypes.c_uint8)), shape=(n * pitch,)).reshape(n, pitch)[:, :cap_]
            return int(fill(first, n, a))
        return self._run(BatchIo(FILL_FN(c_fill), self._sink(on_push, want_lines), None, 0, 0, int(self_staged)))

    def _sink(self, on_push, want_lines=True):
        if on_push is None:
            return LINES_FN()

        def c_lines(user, first, n, lines, n_lines, text, timing):
            recs = None
            if self.cfg.channel_activity:              # the bursts of the collect these lines came with: Batch.bursts[first stream], stream counted from it
                p = ctypes.POINTER(Burst)()
                nb = lib().wmbus_batch_activity(self._h, first, ctypes.byref(p))
                self.bursts.setdefault(first, []).extend(p[k].as_dict() for k in range(nb))
            if want_lines:
                recs = []
                for k in range(n_lines):
                    ln = lines[k]
                    recs.append(dict(stream=ln.stream, channel=ln.channel, chain=ln.chain, algo=ln.algo, crc_ok=ln.crc_ok, sample=ln.sample,
                                     text=ctypes.string_at(text + ln.text_off, ln.text_len).decode()))
                if self.cfg.line_levels:               # the accessor is valid during this callback: every record gets its level
                    p = ctypes.POINTER(Level)()
                    assert lib().wmbus_batch_line_levels(self._h, first, ctypes.byref(p)) == n_lines
                    for k, r in enumerate(recs):
                        r["level"] = p[k].as_dict()
                if self.cfg.crc_repair:                # the same for the repair records
                    p = ctypes.POINTER(Repair)()
                    assert lib().wmbus_batch_line_repairs(self._h, first, ctypes.byref(p)) == n_lines
                    for k, r in enumerate(recs):
                        r["repair"] = p[k].as_dict()
                if self.cfg.s1_rescue:                 # the same for the rescue records
                    p = ctypes.POINTER(Rescue)()
                    assert lib().wmbus_batch_line_rescues(self._h, first, ctypes.byref(p)) == n_lines
                    for k, r in enumerate(recs):
                        r["rescue"] = p[k].as_dict()
                if self.cfg.line_quality:              # the same for the quality records
                    p = ctypes.POINTER(Quality)()
                    assert lib().wmbus_batch_line_quality(self._h, first, ctypes.byref(p)) == n_lines
                    for k, r in enumerate(recs):
                        r["quality"] = p[k].as_dict()
                if self.cfg.line_power:                # the same for the power records
                    p = ctypes.POINTER(Power)()
                    assert lib().wmbus_batch_line_power(self._h, first, ctypes.byref(p)) == n_lines
                    for k, r in enumerate(recs):
                        r["power"] = p[k].as_dict()
            on_push(first, n, recs, timing.contents.as_dict())
        return LINES_FN(c_lines)

    def _run(self, io):
        st = BatchStats()
        self._io = io                                       # the callbacks must outlive the call
        self._chk(lib().wmbus_batch_run(self._h, ctypes.byref(io), ctypes.byref(st)))
        return dict(samples=int(st.samples), lines=int(st.lines), seconds=float(st.seconds), pushes=int(st.pushes), warnings=int(st.warnings))


class Receiver:
    """`n_streams` captures through the GPU back end, in lock step.

    Keyword arguments mirror the reference's switches: decimation (-d), simultaneous (-s),
    accurate_atan (not -a), remove_dc (-o), t1c1 / s1 (not -p T / -p S), rla (-r), time2 (-t),
    show_algorithm (-v).

    input_channel_hz=[f0, f1, ...] (up to MAX_CHANNELS signed offsets in Hz, spelled as input_shift_hz): every capture is a wideband
    capture decoded once per channel.  stage() / push() / device_input() / read_input_dc() / read_input_gain() still count captures;
    the pipeline behind the input stage is n_streams x channels wide and read_resampled() / read_tap() / read_chips() take the
    pipeline stream v = capture * channels + channel; lines() records carry `stream` (the capture) and `channel`; run() returns one
    text per PIPELINE STREAM v, not per capture.
    """

    def __init__(self, n_streams=1, **kw):
        L = lib()
        c = _make_cfg(n_streams=n_streams, **kw)
        self.cfg = c
        self.n_streams = n_streams
        self.n_channels = max(1, int(c.input_channels))
        self._h = ctypes.c_void_p()
        rc = L.wmbus_open(ctypes.byref(c), ctypes.byref(self._h))
        if rc:
            msg = L.wmbus_last_error(self._h).decode() if self._h else "allocation failed"
            L.wmbus_close(self._h)
            self._h = None
            raise WmbusError(f"wmbus_open failed ({rc}): {msg}")

    @classmethod
    def _view(cls, handle, n_streams, n_channels=1):
        """A Receiver over a context someone else owns (a wmbus_batch): never closed from here."""
        r = cls.__new__(cls)
        r._h, r._borrowed, r.n_streams, r.cfg, r.n_channels = ctypes.c_void_p(handle), True, n_streams, None, max(1, int(n_channels))
        return r

    def close(self):
        if getattr(self, "_h", None) and not getattr(self, "_borrowed", False):
            lib().wmbus_close(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise WmbusError(f"error {rc}: {lib().wmbus_last_error(self._h).decode()}")

    def device_input(self, stream):
        return lib().wmbus_device_input(self._h, stream)

    def stage(self, stream, cu8):
        cu8 = np.ascontiguousarray(cu8, dtype=np.uint8)
        self._chk(lib().wmbus_stage(self._h, stream, cu8.ctypes.data, cu8.size))

    def process(self, nbytes):
        self._chk(lib().wmbus_process(self._h, nbytes))

    def collect(self):
        """Returns the datagram text of the push, streams in order, reference stdout order within."""
        L = lib()
        self._chk(L.wmbus_collect(self._h))
        n = ctypes.c_size_t()
        p = L.wmbus_lines_text(self._h, ctypes.byref(n))
        return ctypes.string_at(p, n.value).decode() if n.value else ""

    def lines(self):
        L = lib()
        p = ctypes.POINTER(Line)()
        n = L.wmbus_lines(self._h, ctypes.byref(p))
        sz = ctypes.c_size_t()
        t = L.wmbus_lines_text(self._h, ctypes.byref(sz))
        text = ctypes.string_at(t, sz.value) if sz.value else b""
        return [dict(stream=p[i].stream, channel=p[i].channel, chain=p[i].chain, algo=p[i].algo, crc_ok=p[i].crc_ok, sample=p[i].sample,
                     text=text[p[i].text_off:p[i].text_off + p[i].text_len].decode()) for i in range(n)]

    def line_levels(self):
        """The level records of the last push's lines, in the order of lines() (a context opened with line_levels=1; else [])."""
        p = ctypes.POINTER(Level)()
        n = lib().wmbus_line_levels(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def line_power(self):
        """The power records of the last push's lines, in the order of lines() (a context opened with line_power=1; else [])."""
        p = ctypes.POINTER(Power)()
        n = lib().wmbus_line_power(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def line_repairs(self):
        """The repair records of the last push's lines, in the order of lines() (a context opened with crc_repair=1; else [])."""
        p = ctypes.POINTER(Repair)()
        n = lib().wmbus_line_repairs(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def line_rescues(self):
        """The rescue records of the last push's lines, in the order of lines() (a context opened with s1_rescue=1; else [])."""
        p = ctypes.POINTER(Rescue)()
        n = lib().wmbus_line_rescues(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def rescue_stats(self):
        """(subjects a decoder took, those of them that gave a line) of the last push (s1_rescue=1; else (0, 0))."""
        s, r = ctypes.c_uint(), ctypes.c_uint()
        lib().wmbus_rescue_stats(self._h, ctypes.byref(s), ctypes.byref(r))
        return int(s.value), int(r.value)

    def line_quality(self):
        """The quality records of the last push's lines, in the order of lines() (a context opened with line_quality=1; else [])."""
        p = ctypes.POINTER(Quality)()
        n = lib().wmbus_line_quality(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def activity(self):
        """The bursts the last collect delivered (a context opened with channel_activity=1; else []): dicts of first_block, blocks, mean,
        floor, stream, channel, chain; rows ascending, first_block ascending."""
        p = ctypes.POINTER(Burst)()
        n = lib().wmbus_activity(self._h, ctypes.byref(p))
        return [p[i].as_dict() for i in range(n)]

    def activity_progress(self):
        """The level blocks of the stream the collects so far have taken in (channel_activity=1; else 0)."""
        return int(lib().wmbus_activity_progress(self._h))

    def read_waterfall(self, capture, max_rows=1 << 20):
        """(rows uint32 [n, 32], first_block): the band rows of the last push of one capture (a context with line_power): band j of a row
        holds bins [16 j, 16 j + 16) of that level block's spectrum, Fin / 32 wide, ascending from -Fin / 2."""
        rows = np.zeros((max_rows, 32), np.uint32)
        first = ctypes.c_uint64()
        n = lib().wmbus_read_waterfall(self._h, capture, rows.ctypes.data, ctypes.byref(first), max_rows)
        if n < 0:
            raise WmbusError(f"read_waterfall failed: {n}: {lib().wmbus_last_error(self._h).decode()}")
        return rows[:n].copy(), int(first.value)

    def read_channel_power(self, chain, stream, max_blocks=1 << 20):
        """(P uint32 [n], first_block): the channel power of pipeline row (chain, stream) over the level blocks of the last push."""
        p = np.zeros(max_blocks, np.uint32)
        first = ctypes.c_uint64()
        n = lib().wmbus_read_channel_power(self._h, chain, stream, p.ctypes.data, ctypes.byref(first), max_blocks)
        if n < 0:
            raise WmbusError(f"read_channel_power failed: {n}: {lib().wmbus_last_error(self._h).decode()}")
        return p[:n].copy(), int(first.value)

    def lines_count(self):
        return int(lib().wmbus_lines(self._h, None))

    def timing(self):
        t = Timing()
        self._chk(lib().wmbus_get_timing(self._h, ctypes.byref(t)))
        return t.as_dict()

    def push(self, streams):
        """Stage one equally long array of raw bytes (uint8; cu8 unless input_format says otherwise) per stream, process, decode;
        returns the text."""
        n = None
        for s, a in enumerate(streams):
            a = np.ascontiguousarray(a, dtype=np.uint8)
            n = a.size if n is None else n
            assert a.size == n and n % BLOCK_BYTES == 0
            self.stage(s, a)
        self.process(n)
        return self.collect()

    def run(self, cu8, push_bytes=None):
        """Whole capture(s) through the receiver in pushes of `push_bytes`; partial tail dropped
        like the reference does at EOF (rtl_wmbus.c:1304-1308).  cu8: one array or a list.  Returns one text per capture -- with
        input_channel_hz one per pipeline stream v = capture * channels + channel."""
        streams = [cu8] if isinstance(cu8, np.ndarray) and cu8.ndim == 1 else list(cu8)
        streams = [np.ascontiguousarray(a, dtype=np.uint8) for a in streams]
        total = streams[0].size // BLOCK_BYTES * BLOCK_BYTES
        step = push_bytes or self.cfg.max_push_bytes
        per_stream = [[] for _ in range(len(streams) * self.n_channels)]
        for off in range(0, total, step):
            n = min(step, total - off)
            self.push([a[off:off + n] for a in streams])
            for ln in self.lines():
                per_stream[ln["stream"] * self.n_channels + ln["channel"]].append(ln["text"])
        return ["".join(x) for x in per_stream]

    def read_tap(self, what, chain, stream, n):
        dt = np.float32 if what == "dphi" else np.uint8
        out = np.zeros(n, dt)
        r = lib().wmbus_read_tap(self._h, what.encode(), chain, stream, out.ctypes.data, n)
        if r < 0:
            raise WmbusError(f"read_tap({what}) failed: {r}")
        return out[:r]

    def read_resampled(self, stream, cap=None):
        """The cu8 bytes the last push handed to the pipeline (keep_taps and a context that resamples or converts)."""
        cap = cap or (int(self.cfg.max_push_bytes) * 2 + 8192 if self.cfg is not None else 1 << 24)
        out = np.zeros(cap, np.uint8)
        r = lib().wmbus_read_resampled(self._h, stream, out.ctypes.data, cap)
        if r < 0:
            raise WmbusError(f"read_resampled failed: {r}: {lib().wmbus_last_error(self._h).decode()}")
        return out[:r]

    def read_input_dc(self, stream, cap=None):
        """int16 [n, 2]: {dc_I, dc_Q} the DC blocker subtracted in each level block (512 input samples) of the last push (a context
        with input_dc)."""
        cap = cap or (int(self.cfg.max_push_bytes) // 1024 + 1 if self.cfg is not None else 1 << 16)
        out = np.zeros((cap, 2), np.int16)
        r = lib().wmbus_read_input_dc(self._h, stream, out.ctypes.data, cap)
        if r < 0:
            raise WmbusError(f"read_input_dc failed: {r}: {lib().wmbus_last_error(self._h).decode()}")
        return out[:r]

    def read_input_gain(self, stream, cap=None):
        """uint16 [n]: the gain g (as input_gain_q8 counts it for the 8-bit formats; x 1 / 2^16 for cs16 / cf32) the AGC gave each level
        block (512 input samples) of the last push (a context with input_agc)."""
        cap = cap or (int(self.cfg.max_push_bytes) // 1024 + 1 if self.cfg is not None else 1 << 16)
        out = np.zeros(cap, np.uint16)
        r = lib().wmbus_read_input_gain(self._h, stream, out.ctypes.data, cap)
        if r < 0:
            raise WmbusError(f"read_input_gain failed: {r}: {lib().wmbus_last_error(self._h).decode()}")
        return out[:r]

    def read_spectrum(self, stream, reset=False):
        """(sum uint64 [512], peak uint32 [512], blocks): the survey of capture `stream` over every push since the context was opened or
        the capture's accumulators were last reset (a context with input_spectrum); bin b lies at (b - 256) Fin / 512.  Call it when no
        push is in flight; reset=True zeroes the capture's accumulators behind the read.  With input_spectrum_age = A the three are the
        VIEW: the level blocks of the stream's current epoch of 2^A level blocks and of the one before it (and behind the last reset)."""
        total, peak, blocks = np.zeros(SPECTRUM_BINS, np.uint64), np.zeros(SPECTRUM_BINS, np.uint32), ctypes.c_uint64()
        r = lib().wmbus_read_spectrum(self._h, stream, total.ctypes.data, peak.ctypes.data, ctypes.byref(blocks), int(bool(reset)))
        if r < 0:
            raise WmbusError(f"read_spectrum failed: {r}: {lib().wmbus_last_error(self._h).decode()}")
        return total, peak, int(blocks.value)

    def read_input_afc(self, stream):
        """dict(shift_hz, locked, changes, ratio_q8): the lock the last push of capture `stream` was rotated with (a context with
        input_afc).  Call it when no push is in flight.  With input_spectrum_age the lock follows the survey's last two epochs.  On a
        context with input_channel_afc_hz `stream` is the pipeline stream capture x channels + channel; a fixed channel reads its own
        input_channel_hz, unlocked."""
        out = Afc()
        r = lib().wmbus_read_input_afc(self._h, stream, ctypes.byref(out))
        if r < 0:
            raise WmbusError(f"read_input_afc failed: {r}: {lib().wmbus_last_error(self._h).decode()}")
        return out.as_dict()

    def resampler_launches(self):
        return int(lib().wmbus_resampler_launches(self._h))

    def read_chips(self, chain, algo, stream, cap=1 << 22):
        w = np.zeros(cap, np.uint32)
        pos = np.zeros(cap, np.uint64)
        r = lib().wmbus_read_chips(self._h, chain, algo, stream, w.ctypes.data, pos.ctypes.data, cap)
        if r < 0:
            raise WmbusError(f"read_chips failed: {r}")
        if r > cap:
            raise WmbusError("read_chips: capacity too small")
        return w[:r], pos[:r]


# ---- synthetic captures (host-only helper library) -------------------------------------------------
class SynthCfg(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("fs_khz", ctypes.c_uint), ("noise_sigma", ctypes.c_double),
                ("amplitude", ctypes.c_double), ("frames_per_s", ctypes.c_double), ("kinds", ctypes.c_uint),
                ("l_min", ctypes.c_int), ("l_max", ctypes.c_int), ("t1c1_center_khz", ctypes.c_double),
                ("s1_center_khz", ctypes.c_double), ("max_offset_khz", ctypes.c_double)]


class SynthFrame(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("n_samples", ctypes.c_uint32), ("start_sample", ctypes.c_uint64),
                ("len", ctypes.c_uint16), ("complete", ctypes.c_uint8), ("pad", ctypes.c_uint8),
                ("telegram", ctypes.c_uint8 * 256)]


T1, C1A, C1B, S1 = 1, 2, 4, 8
_synth = None


def _synth_lib():
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise WmbusError(f"{SYNTH_PATH} is missing: run make -C rtl-wmbus_amd")
        L = ctypes.CDLL(SYNTH_PATH)
        L.wmsynth_default_cfg.argtypes = [ctypes.POINTER(SynthCfg)]
        L.wmsynth_generate.restype = ctypes.c_size_t
        L.wmsynth_generate.argtypes = [ctypes.POINTER(SynthCfg), ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(SynthFrame), ctypes.c_size_t]
        _synth = L
    return _synth


def synth_capture(seed, n_samples, fs_khz=1600, kinds=T1 | C1A | C1B, frames_per_s=20.0, amplitude=60.0,
                  noise_sigma=3.0, t1c1_center_khz=0.0, s1_center_khz=0.0, l_min=10, l_max=60, out=None,
                  max_frames=1024):
    """SURVEY.md section 8(d) recipe.  Returns (cu8 uint8[2*n_samples], [frame dicts])."""
    L = _synth_lib()
    c = SynthCfg()
    L.wmsynth_default_cfg(ctypes.byref(c))
    c.seed, c.fs_khz, c.kinds, c.frames_per_s = seed, fs_khz, kinds, frames_per_s
    c.amplitude, c.noise_sigma, c.t1c1_center_khz, c.s1_center_khz = amplitude, noise_sigma, t1c1_center_khz, s1_center_khz
    c.l_min, c.l_max = l_min, l_max
    buf = out if out is not None else np.empty(2 * n_samples, np.uint8)
    fr = (SynthFrame * max_frames)()
    k = L.wmsynth_generate(ctypes.byref(c), buf.ctypes.data, n_samples, fr, max_frames)
    frames = [dict(kind=fr[i].kind, start=fr[i].start_sample, n=fr[i].n_samples, complete=bool(fr[i].complete),
                   telegram=bytes(fr[i].telegram[:fr[i].len])) for i in range(min(k, max_frames))]
    return buf, frames
