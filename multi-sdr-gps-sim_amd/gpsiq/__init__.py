"""gpsiq — Python host binding of libgpsiq (the C-ABI in include/gpsiq.h).

The shared library holds the hand-written gfx950 kernels; this module only marshals
numpy descriptors and raw device pointers (e.g. ``torch.Tensor.data_ptr()``) into it.
There is no fallback: if libgpsiq.so is missing the import fails, and without a GPU
``Context()`` raises.
"""
import ctypes as C
import os

import numpy as np

from .abi import (CHAN_DTYPE, QCHAN_DTYPE, SC08, SC16, SINK_HACKRF, SINK_IQFILE,  # noqa: F401
                  SINK_PLUTOSDR, HACKRF_CHUNK, MAX_CHAN, elem_dtype, EPHEM_DTYPE, IONO_DTYPE, TRACK_DTYPE,
                  NAV_EPH_DTYPE, NAV_UTC_DTYPE, NAV_ALM_DTYPE, NAV_STATE_DTYPE, RINEX_EPH_DTYPE, PATCH_DTYPE,
                  NCO_FIXED, NCO_REFERENCE, SHARD_CARRY_DTYPE, DESPREAD_SUM_DTYPE, BLOCK_STATS_DTYPE, ACQ_PEAK_DTYPE,
                  FOLLOW_STATE_DTYPE, FOLLOW_EPOCH_DTYPE, FOLLOW_CFG_DTYPE, MIX_STREAM, MIX_ROTATED, MIX_TONE, MIX_MAX_TERMS)

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPSIQ_LIB: another build of the library (tests/test_gpu_build.py loads the one it has just compiled on the GPU box)
LIB_PATH = os.environ.get("GPSIQ_LIB") or os.path.join(_HERE, "libgpsiq.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or make -C multi-sdr-gps-sim_amd/csrc); gpsiq has no non-HIP path")



def _preload_shared_hip_runtime():
    """PyTorch wheels carry their own libamdhip64.so (SONAME libamdhip64.so.7) and load it by
    file name, so a process that loaded /opt/rocm's copy first ends up with two HIP/HSA
    runtimes and the second one to initialise sees no device.  When torch is installed,
    load ITS runtime first (without importing torch) so libgpsiq.so binds to the same one."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


_preload_shared_hip_runtime()
_lib = C.CDLL(LIB_PATH)
# the rows either side of the path (include/gpsiq_rows.h, gpsiq_extras.h): a host-only library of its own that runs on the first
# one's worker pool and error text (its NEEDED entry "libgpsiq.so" is satisfied by the library just loaded, whatever its path)
ROWS_PATH = os.path.join(os.path.dirname(LIB_PATH), "libgpsiq_rows.so")
if not os.path.exists(ROWS_PATH):
    ROWS_PATH = os.path.join(_HERE, "libgpsiq_rows.so")
if not os.path.exists(ROWS_PATH):
    raise ImportError(f"{ROWS_PATH} not built: make -C multi-sdr-gps-sim_amd/csrc builds it next to libgpsiq.so")
_rows = C.CDLL(ROWS_PATH)


class GpsiqError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"gpsiq error {code}: {text}")
        self.code = code


def _sig(name, restype, *argtypes):
    """A function of the C-ABI (an exported symbol: include/gpsiq.h in libgpsiq.so, include/gpsiq_rows.h and gpsiq_extras.h in
    libgpsiq_rows.so), or of the library's plumbing (csrc/gpsiq_plumbing.h: hidden symbols, resolved through the one exported
    entry gpsiq_plumbing(name))."""
    f = getattr(_lib, name, None) or getattr(_rows, name, None)
    if f is None:
        _lib.gpsiq_plumbing.restype = C.c_void_p
        _lib.gpsiq_plumbing.argtypes = [C.c_char_p]
        addr = _lib.gpsiq_plumbing(name.encode())
        if not addr:
            raise AttributeError(f"{name}: exported by neither libgpsiq.so nor libgpsiq_rows.so, and no plumbing entry of that name")
        return C.CFUNCTYPE(restype, *argtypes)(addr)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_vp, _i, _d, _sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
_version = _sig("gpsiq_version", C.c_char_p)
_last_error = _sig("gpsiq_last_error", C.c_char_p)
_kernels_id = _sig("gpsiq_kernels_id", C.c_char_p)
_prn_code = _sig("gpsiq_prn_code", _i, _i, _vp)
_carrier_table = _sig("gpsiq_carrier_table", None, _vp, _vp)
_quantize = _sig("gpsiq_quantize", _i, _vp, _i, _d, _i, _vp, _vp, _vp)
_create = _sig("gpsiq_create", _i, C.POINTER(_vp), _i)
_destroy = _sig("gpsiq_destroy", None, _vp)
_generate_block = _sig("gpsiq_generate_block", _i, _vp, _vp, _i, _i, _d, _i, _vp, _vp)
_generate_block_async = _sig("gpsiq_generate_block_async", _i, _vp, _vp, _i, _i, _d, _i, _vp, _vp)
_wait = _sig("gpsiq_wait", _i, _vp)
_generate_batch = _sig("gpsiq_generate_batch", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _i, _vp)
_generate_quantized = _sig("gpsiq_generate_quantized", _i, _vp, _vp, _i, _i, _i, _i, _vp, _i)
_generate_seeded = _sig("gpsiq_generate_seeded", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i)
_quantize_batch = _sig("gpsiq_quantize_batch", _i, _vp, _i, _i, _d, _i, _vp, _vp, _vp)
_reference_batch = _sig("gpsiq_reference_batch", _i, _vp, _i, _i, _d, _i, _vp, _vp, _i, C.POINTER(C.c_int), _vp)
_reference_chain = _sig("gpsiq_reference_chain", _i, _vp, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp)
_reference_seeded = _sig("gpsiq_reference_seeded", _i, _vp, _i, _i, _d, _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int))
_reference_stats = _sig("gpsiq_reference_stats", None, _vp)
_chain_inputs = _sig("gpsiq_chain_inputs", None, _vp, _i, _vp)
_chain_maps = _sig("gpsiq_chain_maps", _i, _vp, _i, _i, _d, _i, _vp, _i, _vp, _vp)
_chain_maps_device = _sig("gpsiq_chain_maps_device", _i, _vp, _vp, _i, _i, _d, _i, _vp, _i, _vp, _vp, C.POINTER(C.c_float))
_chain_link = _sig("gpsiq_chain_link", _i, _vp, _vp, _i, _i, _d, _i, _vp, _vp, _vp, _vp, _vp)
_chain_summary = _sig("gpsiq_chain_summary", _i, _vp, _i, _i, _d, _i, _vp, _vp)
_chain_fold = _sig("gpsiq_chain_fold", _i, _vp, _i, _i, _vp)
_chain_range = _sig("gpsiq_chain_range", _i, _vp, _vp, _i, _i, _d, _i, _vp)
_chain_range_fold = _sig("gpsiq_chain_range_fold", _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp)
_chain_stats = _sig("gpsiq_chain_stats", None, _vp)
_set_patches = _sig("gpsiq_set_patches", _i, _vp, _vp, _i)
_set_nco_mode = _sig("gpsiq_set_nco_mode", _i, _vp, _i)
_generate_batch_multi = _sig("gpsiq_generate_batch_multi", _i, _vp, _i, _vp, _i, _i, _i, _d, _i, _vp, _vp, _vp)
_shard_carry = _sig("gpsiq_shard_carry", _i, _vp, _i, _i, _i, _vp)
_shard_seed = _sig("gpsiq_shard_seed", _i, _vp, _i, _i, _i, _vp, _i)
_shard_range = _sig("gpsiq_shard_range", _i, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int))
_set_descriptors = _sig("gpsiq_set_descriptors", _i, _vp, _vp, _i, _i)
_launch = _sig("gpsiq_launch", _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i)
_synchronize = _sig("gpsiq_synchronize", _i, _vp, _vp)
_time_launches = _sig("gpsiq_time_launches", _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i, _i, C.POINTER(C.c_float))
_host_alloc = _sig("gpsiq_host_alloc", _vp, _sz)
_host_free = _sig("gpsiq_host_free", None, _vp)
_track_init = _sig("gpsiq_track_init", _i, _vp, _vp, _i, _d, _vp, _vp, _i)
_sat_visibility = _sig("gpsiq_sat_visibility", _i, _vp, _i, _d, _vp, _d, _vp)
_refresh_batch = _sig("gpsiq_refresh_batch", _i, _vp, _vp, _i, _d, _vp, _i, _i, _i, _vp, _vp, _i)
_refresh_epochs = _sig("gpsiq_refresh_epochs", _i, _vp, _vp, _i, _d, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _i)
_almanac_read_sem = _sig("gpsiq_almanac_read_sem", _i, C.c_char_p, _vp)
_rinex_overwrite_time = _sig("gpsiq_rinex_overwrite_time", _i, _vp, _i, _vp, _i, _d)
_ecef_add_neu = _sig("gpsiq_ecef_add_neu", None, _vp, _vp, _vp)
_date_to_gps = _sig("gpsiq_date_to_gps", None, _i, _i, _i, _i, _i, _d, _vp, _vp)
_gps_to_date = _sig("gpsiq_gps_to_date", None, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp)
_refresh_epochs_q = _sig("gpsiq_refresh_epochs_quantized", _i, _vp, _vp, _i, _d, _vp, _i, _i, _i, _vp, _vp, _i, _d, _i, _vp, _i)
_llh_to_ecef = _sig("gpsiq_llh_to_ecef", None, _vp, _vp)
_ecef_to_llh = _sig("gpsiq_ecef_to_llh", None, _vp, _vp)
_motion_read_csv = _sig("gpsiq_motion_read_csv", _i, C.c_char_p, _vp, _i)
_nav_parity = _sig("gpsiq_nav_parity", C.c_uint32, C.c_uint32, _i)
_nav_subframes = _sig("gpsiq_nav_subframes", _i, _vp, _vp, _vp, _vp)
_nav_message = _sig("gpsiq_nav_message", _i, _vp, _i, _d, _i, _vp)
_nav_roll = _sig("gpsiq_nav_roll", _i, _vp, _i, _i, _d, _vp)
_rinex_read = _sig("gpsiq_rinex_read", _i, C.c_char_p, _i, _vp, _vp)
_rinex_select = _sig("gpsiq_rinex_select", _i, _vp, _i, _i, _d)
_device_eval_stats = _sig("gpsiq_device_eval_stats", None, _vp)
_device_eval_host_ms = _sig("gpsiq_device_eval_host_ms", _d, _vp)
_num_variants = _sig("gpsiq_num_variants", _i)
_variant_name = _sig("gpsiq_variant_name", C.c_char_p, _i)
_set_noise = _sig("gpsiq_set_noise", _i, _vp, _vp)
_noise_state = _sig("gpsiq_noise_state", _i, _vp, _vp)
_noise_host = _sig("gpsiq_noise_host", _i, C.c_uint64, _d, C.c_uint64, _i, _vp)
_noise_sigma_for_cn0 = _sig("gpsiq_noise_sigma_for_cn0", _d, _d, _d, _d)
_set_level = _sig("gpsiq_set_level", _i, _vp, _vp)
_composite_rms = _sig("gpsiq_composite_rms", _d, _vp, _i, _d)
_level_mult = _sig("gpsiq_level_mult", C.c_uint32, _d, _d)
_despread = _sig("gpsiq_despread", _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_float))
_despread_last_plan = _sig("gpsiq_despread_last_plan", _i, _vp, _vp)
_cn0_estimate = _sig("gpsiq_cn0_estimate", _i, _vp, _i, _i, _d, C.POINTER(_d), C.POINTER(_d))
_packed_block_bytes = _sig("gpsiq_packed_block_bytes", _sz, _i, _i)
_pack = _sig("gpsiq_pack", _i, _vp, _i, _i, _i, _vp, _sz, _i, _vp, _sz, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_unpack = _sig("gpsiq_unpack", _i, _vp, _i, _i, _i, _vp, _sz, _i, _vp, _sz, _vp, C.POINTER(C.c_float))
_generate_batch_packed = _sig("gpsiq_generate_batch_packed", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _sz, _vp)
_pack_last_plan = _sig("gpsiq_pack_last_plan", _i, _vp, _vp)
_acquire = _sig("gpsiq_acquire", _i, _vp, _i, _i, _vp, _vp, _vp, _i, C.c_uint64, C.c_int64, C.c_int64, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_float))
_acquire_last_plan = _sig("gpsiq_acquire_last_plan", _i, _vp, _vp, _vp)
_acquire_steps = _sig("gpsiq_acquire_steps", _i, _d, _d, _d, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_acquire_decide = _sig("gpsiq_acquire_decide", _i, _vp, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_d))
_follow = _sig("gpsiq_follow", _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, C.POINTER(C.c_float))
_follow_last_plan = _sig("gpsiq_follow_last_plan", _i, _vp, _vp)
_follow_gains = _sig("gpsiq_follow_gains", _i, _d, _d, _d, _d, _vp)
_follow_bits = _sig("gpsiq_follow_bits", _i, _vp, _i, _i, C.POINTER(_i), _vp, _i, C.POINTER(_i))
_filter = _sig("gpsiq_filter", _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, C.POINTER(_i), C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_filter_span = _sig("gpsiq_filter_span", _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i))
_filter_design = _sig("gpsiq_filter_design", _i, _d, _d, _i, _i, _vp)
_generate_batch_filtered = _sig("gpsiq_generate_batch_filtered", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _i, _i, _i, _i, _vp, _sz, C.POINTER(C.c_uint64), _vp)
_filter_last_plan = _sig("gpsiq_filter_last_plan", _i, _vp, _vp)
_spectrum = _sig("gpsiq_spectrum", _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.POINTER(_i), C.POINTER(C.c_float))
_spectrum_span = _sig("gpsiq_spectrum_span", _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i))
_spectrum_min_shift = _sig("gpsiq_spectrum_min_shift", _i, _i, _i, _i, _i)
_spectrum_scale = _sig("gpsiq_spectrum_scale", _i, _i, _i, _i, _i, _d, C.POINTER(_d))
_spectrum_last_plan = _sig("gpsiq_spectrum_last_plan", _i, _vp, _vp)
_mix = _sig("gpsiq_mix", _i, _vp, _i, C.c_uint64, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_mix_advance = _sig("gpsiq_mix_advance", _i, _vp, _i, C.c_uint64)
_mix_tone = _sig("gpsiq_mix_tone", _i, _d, _d, _d, _d, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32))
_mix_gain = _sig("gpsiq_mix_gain", _i, _d, _i, _i, C.POINTER(C.c_int32))
_generate_batch_mixed = _sig("gpsiq_generate_batch_mixed", _i, _vp, _vp, _i, _i, _i, _d, _i, C.c_int32, _vp, _i, C.c_uint64, _i, _i, _vp, _sz,
                             C.POINTER(C.c_uint64), _vp)
_mix_last_plan = _sig("gpsiq_mix_last_plan", _i, _vp, _vp)
_u64 = C.c_uint64
_resample = _sig("gpsiq_resample", _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _u64, _u64, _i, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64),
                 C.POINTER(_u64), C.POINTER(C.c_float))
_resample_span = _sig("gpsiq_resample_span", _i, _u64, _u64, _u64, C.POINTER(_u64), C.POINTER(_u64))
_resample_step = _sig("gpsiq_resample_step", _i, _d, _d, _d, C.POINTER(_u64))
_resample_design = _sig("gpsiq_resample_design", _i, _u64, _d, _i, _i, _i, _vp)
_generate_batch_resampled = _sig("gpsiq_generate_batch_resampled", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _i, _i, _i, _i, _u64, _u64, _i, _vp, _u64,
                                 C.POINTER(_u64), C.POINTER(_u64), _vp)
_resample_last_plan = _sig("gpsiq_resample_last_plan", _i, _vp, _vp)
_agc = _sig("gpsiq_agc", _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_float))
_agc_mult = _sig("gpsiq_agc_mult", _i, _vp, _u64, _u64, C.POINTER(C.c_uint32))
_agc_span = _sig("gpsiq_agc_span", _i, _u64, _i, C.c_uint32, C.POINTER(_u64), C.POINTER(C.c_uint32))
_generate_batch_agc = _sig("gpsiq_generate_batch_agc", _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _vp, _sz, C.POINTER(_u64), C.POINTER(_u64), _vp)
_agc_last_plan = _sig("gpsiq_agc_last_plan", _i, _vp, _vp)
_agc_last_ms = _sig("gpsiq_agc_last_ms", _i, _vp, _vp)
_cfilter = _sig("gpsiq_cfilter", _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, C.POINTER(_i), C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_cfilter_last_plan = _sig("gpsiq_cfilter_last_plan", _i, _vp, _vp)
_notch_find = _sig("gpsiq_notch_find", _i, _vp, _i, _d, _d, _i, _vp, _vp, C.POINTER(_i))
_notch_design = _sig("gpsiq_notch_design", _i, _d, _vp, _i, _d, _i, _i, _vp)
_array_cov = _sig("gpsiq_array_cov", _i, _vp, _i, _vp, _i, _i, _vp, _vp, C.POINTER(C.c_float))
_array_combine = _sig("gpsiq_array_combine", _i, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_array_steer = _sig("gpsiq_array_steer", _i, _vp, _i, _d, _d, _vp)
_array_weights = _sig("gpsiq_array_weights", _i, _vp, _i, C.c_uint64, _vp, _d, _i, _vp)
_array_last_plan = _sig("gpsiq_array_last_plan", _i, _vp, _vp)
ARRAY_MAX_ELEM = 8
_stap_cov = _sig("gpsiq_stap_cov", _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_float))
_stap_combine = _sig("gpsiq_stap_combine", _i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float))
_stap_weights = _sig("gpsiq_stap_weights", _i, _vp, _i, _i, C.c_uint64, _vp, _i, _d, _i, _vp)
_stap_last_plan = _sig("gpsiq_stap_last_plan", _i, _vp, _vp)
STAP_MAX_TAPS = 8
STAP_MAX_ROWS = 32
_stap_beams = _sig("gpsiq_stap_beams", _i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_float))
_stap_beam_weights = _sig("gpsiq_stap_beam_weights", _i, _vp, _i, _i, C.c_uint64, _vp, _i, _i, _d, _i, _vp)
_stap_beams_last_plan = _sig("gpsiq_stap_beams_last_plan", _i, _vp, _vp)
STAP_MAX_BEAMS = 8


class CTap(C.Structure):
    """gpsiq_ctap_t (include/gpsiq_rows.h, "Complex filter and notch"): one complex tap, re + j im."""
    _fields_ = [("re", C.c_int16), ("im", C.c_int16)]


def ctaps(taps):
    """Complex taps as the int16 array [n, 2] (re, im) gpsiq_cfilter takes: from such an array, from a sequence of CTap, or from a ctypes
    array of CTap."""
    if isinstance(taps, C.Array) and getattr(taps, "_type_", None) is CTap:
        return np.frombuffer(taps, dtype=np.int16).reshape(-1, 2).copy()
    if not isinstance(taps, np.ndarray) and len(taps) and isinstance(taps[0], CTap):
        return np.array([(t.re, t.im) for t in taps], dtype=np.int16).reshape(-1, 2)
    a = np.asarray(taps)
    if a.ndim != 2 or a.shape[1] != 2:
        raise GpsiqError(-1, f"complex taps are [n, 2] (re, im), not an array of shape {a.shape}")
    if a.size and (a.min() < -32768 or a.max() > 32767):
        raise GpsiqError(-1, "a complex tap does not fit int16")
    return np.ascontiguousarray(a, dtype=np.int16)


class AgcCfg(C.Structure):
    """gpsiq_agc_cfg_t (include/gpsiq_rows.h, "AGC")."""
    _fields_ = [("window", C.c_int32), ("navg", C.c_int32), ("target_q8", C.c_uint32), ("mult0", C.c_uint32), ("mult_min", C.c_uint32),
                ("mult_max", C.c_uint32), ("blank_thresh", C.c_int32), ("blank_hold", C.c_int32), ("qmax", C.c_int32)]

    def __init__(self, window=1024, navg=16, target_q8=256, mult0=65536, mult_min=1, mult_max=(1 << 24) - 1, blank_thresh=0, blank_hold=0, qmax=127):
        super().__init__(window, navg, target_q8, mult0, mult_min, mult_max, blank_thresh, blank_hold, qmax)


class AgcState(C.Structure):
    """gpsiq_agc_state_t (ibid.): all zeros is a fresh stream."""
    _fields_ = [("wsum", C.c_uint64 * 64), ("wcnt", C.c_uint32 * 64), ("psum", C.c_uint64), ("pcnt", C.c_uint32), ("fill", C.c_uint32),
                ("nring", C.c_uint32), ("hold", C.c_uint32)]

    def as_tuple(self):
        return (tuple(self.wsum), tuple(self.wcnt), int(self.psum), int(self.pcnt), int(self.fill), int(self.nring), int(self.hold))

    def copy(self):
        other = AgcState()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(AgcState))
        return other


class NoiseSettings(C.Structure):
    """gpsiq_noise_t (include/gpsiq.h)."""
    _fields_ = [("seed", C.c_uint64), ("sigma", C.c_double), ("next_block", C.c_uint64)]


class LevelSettings(C.Structure):
    """gpsiq_level_t (include/gpsiq_rows.h)."""
    _fields_ = [("mult", C.c_uint32), ("qmax", C.c_int32)]


class MixTerm(C.Structure):
    """gpsiq_mix_term_t (include/gpsiq_rows.h, "Mix"): one term of Context.mix().  MixTerm.stream / .rotated / .tone build one."""
    _fields_ = [("kind", C.c_int32), ("sample_size", C.c_int32), ("src", C.c_void_p), ("skip", C.c_uint64), ("gain", C.c_int32),
                ("reserved", C.c_int32), ("phase0", C.c_uint64), ("step", C.c_int64), ("rate", C.c_int64), ("sweep_period", C.c_uint32),
                ("sweep_offset", C.c_uint32), ("gate_period", C.c_uint32), ("gate_on", C.c_uint32), ("gate_offset", C.c_uint32),
                ("reserved2", C.c_uint32)]

    @classmethod
    def stream(cls, src, sample_size, gain, skip=0, gate=(0, 0, 0)):
        """t = x: the stream at src (a device or page-locked address), delayed by skip samples; gate: (period, on, offset)."""
        return cls(kind=MIX_STREAM, sample_size=int(sample_size), src=int(src), skip=int(skip), gain=int(gain), gate_period=int(gate[0]),
                   gate_on=int(gate[1]), gate_offset=int(gate[2]))

    @classmethod
    def rotated(cls, src, sample_size, gain, step, skip=0, phase0=0, rate=0, sweep=(0, 0), gate=(0, 0, 0)):
        """t = x (c + j s): the stream at src turned by the NCO (step, rate in 2**-59 cycle; sweep: (period, offset))."""
        return cls(kind=MIX_ROTATED, sample_size=int(sample_size), src=int(src), skip=int(skip), gain=int(gain), phase0=int(phase0) % 2 ** 64,
                   step=int(step), rate=int(rate), sweep_period=int(sweep[0]), sweep_offset=int(sweep[1]), gate_period=int(gate[0]),
                   gate_on=int(gate[1]), gate_offset=int(gate[2]))

    @classmethod
    def tone(cls, gain, step, phase0=0, rate=0, sweep=(0, 0), gate=(0, 0, 0)):
        """t = (c, s): the bare NCO, a tone (rate 0) or a chirp."""
        return cls(kind=MIX_TONE, gain=int(gain), phase0=int(phase0) % 2 ** 64, step=int(step), rate=int(rate), sweep_period=int(sweep[0]),
                   sweep_offset=int(sweep[1]), gate_period=int(gate[0]), gate_on=int(gate[1]), gate_offset=int(gate[2]))


def _mix_terms(terms):
    arr = (MixTerm * max(len(terms), 1))()
    for k, t in enumerate(terms):
        C.memmove(C.byref(arr, k * C.sizeof(MixTerm)), C.byref(t), C.sizeof(MixTerm))
    return arr


def _check(rc):
    if rc < 0:
        raise GpsiqError(rc, _last_error().decode())
    return rc


def _p(a):
    return a.ctypes.data_as(_vp)


def version():
    return _version().decode()


def kernels_id():
    """Identity of the device code in the loaded library (see gpsiq_kernels_id in include/gpsiq.h)."""
    return _kernels_id().decode()


def variants():
    return {_variant_name(v).decode(): v for v in range(_num_variants())}


def prn_code(prn):
    ca = np.zeros(1023, dtype=np.uint8)
    _check(_prn_code(int(prn), _p(ca)))
    return ca


def carrier_table():
    cos = np.zeros(512, dtype=np.int16)
    sin = np.zeros(512, dtype=np.int16)
    _carrier_table(_p(cos), _p(sin))
    return cos, sin


def quantize(ch, fs, nsamp, carry_in=None):
    """One block: gpsiq_chan_t[nchan] -> (gpsiq_qchan_t[nchan], carry_out[nchan])."""
    ch = np.ascontiguousarray(ch, dtype=CHAN_DTYPE)
    q = np.zeros(len(ch), dtype=QCHAN_DTYPE)
    cout = np.zeros(len(ch), dtype=np.uint64)
    cin = None if carry_in is None else np.ascontiguousarray(carry_in, dtype=np.uint64)
    _check(_quantize(_p(ch), len(ch), float(fs), int(nsamp), _p(q), None if cin is None else _p(cin), _p(cout)))
    return q, cout


def quantize_blocks(desc, fs, nsamp, carry0=None):
    """[nblocks][nchan] descriptors -> quantised descriptors with the carrier carried
    exactly from block to block (the rule of gpsiq_generate_batch).  Returns (q, carry_end)."""
    desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
    nb, nc = desc.shape
    q = np.zeros((nb, nc), dtype=QCHAN_DTYPE)
    cin = None if carry0 is None else np.ascontiguousarray(carry0, dtype=np.uint64)
    cout = np.zeros(nc, dtype=np.uint64)
    _check(_quantize_batch(_p(desc), nb, nc, float(fs), int(nsamp), _p(q), None if cin is None else _p(cin), _p(cout)))
    return q, cout


def reference_blocks(desc, fs, nsamp):
    """GPSIQ_NCO_REFERENCE form of quantize_blocks: (q, patches, carr_phase_end).  Every block is seeded from
    the carrier phase the reference's double accumulator holds at its start; patches lists the samples where
    the double path differs from the closed form."""
    desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
    nb, nc = desc.shape
    q = np.zeros((nb, nc), dtype=QCHAN_DTYPE)
    carr = np.zeros(nc, dtype=np.float64)
    n = C.c_int(0)
    cap = 64 + 8 * nb
    while True:
        pt = np.zeros(cap, dtype=PATCH_DTYPE)
        rc = _reference_batch(_p(desc), nb, nc, float(fs), int(nsamp), _p(q), _p(pt), cap, C.byref(n), _p(carr))
        if rc == -2 and n.value > cap:           # GPSIQ_E_RANGE: not enough room
            cap = n.value
            continue
        _check(rc)
        return q, pt[: n.value].copy(), carr


def chain_inputs(desc):
    """gpsiq_chain_inputs: the three fields per channel and block the serial carrier chain reads, [nblocks][nchan] x 24 bytes."""
    from .abi import CHAIN_IN_DTYPE
    desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
    out = np.zeros(desc.shape, dtype=CHAIN_IN_DTYPE)
    _chain_inputs(_p(desc), desc.size, _p(out))
    return out


def reference_chain(cin, fs, nsamp, carr_in=None, prn_in=None):
    """gpsiq_reference_chain: the serial half of GPSIQ_NCO_REFERENCE alone.  cin [nblocks][nchan] (chain_inputs, or any
    subset of its columns: the channels are independent) -> (carr_start[nblocks][nchan], carr_end[nchan], last_prn[nchan])."""
    from .abi import CHAIN_IN_DTYPE
    cin = np.ascontiguousarray(cin, dtype=CHAIN_IN_DTYPE)
    nb, nc = cin.shape
    start = np.zeros((nb, nc), dtype=np.float64)
    end = np.zeros(nc, dtype=np.float64)
    last = np.zeros(nc, dtype=np.int32)
    ci = None if carr_in is None else np.ascontiguousarray(carr_in, dtype=np.float64)
    pi = None if prn_in is None else np.ascontiguousarray(prn_in, dtype=np.int32)
    _check(_reference_chain(_p(cin), nb, nc, float(fs), int(nsamp), None if ci is None else _p(ci), None if pi is None else _p(pi),
                            _p(start), _p(end), _p(last)))
    return start, end, last


def chain_maps(cin, fs, nsamp, start=None, max_stretches=0, ctx=None):
    """gpsiq_chain_maps (ctx given: gpsiq_chain_maps_device): level 1 of the time-parallel carrier chain, the certified map of
    every block -> (maps[nblocks][nchan], end[nchan]) (+ the kernels' milliseconds on a device)."""
    from .abi import CHAIN_IN_DTYPE, CHAIN_EST_DTYPE, CHAIN_MAP_DTYPE
    cin = np.ascontiguousarray(cin, dtype=CHAIN_IN_DTYPE)
    nb, nc = cin.shape
    maps = np.zeros((nb, nc), dtype=CHAIN_MAP_DTYPE)
    end = np.zeros(nc, dtype=CHAIN_EST_DTYPE)
    st = None if start is None else np.ascontiguousarray(start, dtype=CHAIN_EST_DTYPE)
    if ctx is None:
        _check(_chain_maps(_p(cin), nb, nc, float(fs), int(nsamp), None if st is None else _p(st), int(max_stretches), _p(maps), _p(end)))
        return maps, end
    ms = C.c_float(0.0)
    _check(_chain_maps_device(ctx._h, _p(cin), nb, nc, float(fs), int(nsamp), None if st is None else _p(st), int(max_stretches),
                              _p(maps), _p(end), C.byref(ms)))
    return maps, end, float(ms.value)


def chain_link(cin, maps, fs, nsamp, carr_in=None, prn_in=None):
    """gpsiq_chain_link: level 2, the chain itself -> (carr_start[nblocks][nchan], carr_end[nchan], last_prn[nchan]), equal to
    reference_chain's."""
    from .abi import CHAIN_IN_DTYPE, CHAIN_MAP_DTYPE
    cin = np.ascontiguousarray(cin, dtype=CHAIN_IN_DTYPE)
    maps = np.ascontiguousarray(maps, dtype=CHAIN_MAP_DTYPE)
    nb, nc = cin.shape
    assert maps.shape == (nb, nc)
    start = np.zeros((nb, nc), dtype=np.float64)
    end = np.zeros(nc, dtype=np.float64)
    last = np.zeros(nc, dtype=np.int32)
    ci = None if carr_in is None else np.ascontiguousarray(carr_in, dtype=np.float64)
    pi = None if prn_in is None else np.ascontiguousarray(prn_in, dtype=np.int32)
    _check(_chain_link(_p(cin), _p(maps), nb, nc, float(fs), int(nsamp), None if ci is None else _p(ci), None if pi is None else _p(pi),
                       _p(start), _p(end), _p(last)))
    return start, end, last


def chain_summary(cin, fs, nsamp, start=None):
    """gpsiq_chain_summary: what a range of blocks does to every slot's estimator (start None: the phase pass)."""
    from .abi import CHAIN_IN_DTYPE, CHAIN_EST_DTYPE
    cin = np.ascontiguousarray(cin, dtype=CHAIN_IN_DTYPE)
    nb, nc = cin.shape
    out = np.zeros(nc, dtype=CHAIN_EST_DTYPE)
    st = None if start is None else np.ascontiguousarray(start, dtype=CHAIN_EST_DTYPE)
    _check(_chain_summary(_p(cin), nb, nc, float(fs), int(nsamp), None if st is None else _p(st), _p(out)))
    return out


def chain_fold(sums):
    """gpsiq_chain_fold: the estimator state after the ranges sums[0 .. n) ([n][nchan]), i.e. where range n starts."""
    from .abi import CHAIN_EST_DTYPE
    sums = np.ascontiguousarray(sums, dtype=CHAIN_EST_DTYPE)
    n, nc = sums.shape
    out = np.zeros(nc, dtype=CHAIN_EST_DTYPE)
    _check(_chain_fold(_p(sums) if n else None, n, nc, _p(out)))
    return out


def chain_range(cin, maps, fs, nsamp):
    """gpsiq_chain_range: what this range of blocks does to every slot's accumulator as a function of the state it is entered
    with (its maps composed) -> CHAIN_RANGE_DTYPE[nchan]."""
    from .abi import CHAIN_IN_DTYPE, CHAIN_MAP_DTYPE, CHAIN_RANGE_DTYPE
    cin = np.ascontiguousarray(cin, dtype=CHAIN_IN_DTYPE)
    maps = np.ascontiguousarray(maps, dtype=CHAIN_MAP_DTYPE)
    nb, nc = cin.shape
    out = np.zeros(nc, dtype=CHAIN_RANGE_DTYPE)
    _check(_chain_range(_p(cin) if nb else None, _p(maps) if nb else None, nb, nc, float(fs), int(nsamp), _p(out)))
    return out


def chain_range_fold(ranges, true_end=None, true_prn=None, true_known=None):
    """gpsiq_chain_range_fold over ranges[nranges][nchan]: (every state known, carr, prn, known -- each [nranges + 1][nchan]) --
    the accumulator and satellite every range is entered with, the last row: after the whole timeline.  true_end / true_prn
    [nranges][nchan] with true_known[nranges]: the states ranks that have linked their range ended on."""
    from .abi import CHAIN_RANGE_DTYPE
    ranges = np.ascontiguousarray(ranges, dtype=CHAIN_RANGE_DTYPE)
    n, nc = ranges.shape
    carr = np.zeros((n + 1, nc), dtype=np.float64)
    prn = np.zeros((n + 1, nc), dtype=np.int32)
    known = np.zeros((n + 1, nc), dtype=np.uint8)
    te = tp = tk = None
    if true_known is not None:
        te = np.ascontiguousarray(true_end, dtype=np.float64)
        tp = np.ascontiguousarray(true_prn, dtype=np.int32)
        tk = np.ascontiguousarray(true_known, dtype=np.uint8)
        assert te.shape == (n, nc) and tp.shape == (n, nc) and tk.shape == (n,)
    every = _check(_chain_range_fold(_p(ranges) if n else None, n, nc, None if tk is None else _p(te), None if tk is None else _p(tp),
                                     None if tk is None else _p(tk), _p(carr), _p(prn), _p(known)))
    return bool(every), carr, prn, known.astype(bool)


def chain_stats():
    """gpsiq_chain_stats: (blocks linked through their map, blocks walked from their true start) since the process started."""
    out = np.zeros(2, dtype=np.uint64)
    _chain_stats(_p(out))
    return int(out[0]), int(out[1])


def reference_seeded(desc, fs, nsamp, carr_start):
    """gpsiq_reference_seeded: the parallel half -- (q, patches) of blocks whose start states are known."""
    desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
    nb, nc = desc.shape
    st = np.ascontiguousarray(carr_start, dtype=np.float64)
    assert st.shape == (nb, nc)
    q = np.zeros((nb, nc), dtype=QCHAN_DTYPE)
    n = C.c_int(0)
    cap = 64 + 8 * nb
    while True:
        pt = np.zeros(cap, dtype=PATCH_DTYPE)
        rc = _reference_seeded(_p(desc), nb, nc, float(fs), int(nsamp), _p(st), _p(q), _p(pt), cap, C.byref(n))
        if rc == -2 and n.value > cap:
            cap = n.value
            continue
        _check(rc)
        return q, pt[: n.value].copy()


def reference_stats():
    """gpsiq_reference_stats: (states needed, decided from the start state, carrier walks, code walks) since the process started."""
    out = np.zeros(4, dtype=np.uint64)
    _reference_stats(_p(out))
    return tuple(int(v) for v in out)


def device_eval_stats():
    """Since the process started: batch calls taken by the device evaluation, (block, channel) pairs it evaluated, pairs handed
    to the host walker, slots whose chain the host repaired, patches, calls that fell back to the host path."""
    out = np.zeros(6, dtype=np.uint64)
    _device_eval_stats(_p(out))
    return tuple(int(v) for v in out)


def shard_carry(q, nsamp):
    """gpsiq_shard_carry: what this rank's (self-seeded) block range does to each slot's carrier."""
    q = np.ascontiguousarray(q, dtype=QCHAN_DTYPE)
    nb, nc = q.shape
    out = np.zeros(nc, dtype=SHARD_CARRY_DTYPE)
    _check(_shard_carry(_p(q), nb, nc, int(nsamp), _p(out)))
    return out


def shard_seed(q, nsamp, all_carry, rank):
    """gpsiq_shard_seed: add the exact carrier prefix of the ranks before `rank` to q (in place)."""
    assert q.dtype == QCHAN_DTYPE and q.flags.c_contiguous
    nb, nc = q.shape
    allc = np.ascontiguousarray(all_carry, dtype=SHARD_CARRY_DTYPE).reshape(-1, nc)
    _check(_shard_seed(_p(q), nb, nc, int(nsamp), _p(allc), int(rank)))
    return q


def shard_range(nblocks, rank, world):
    """gpsiq_shard_range: the contiguous block range [begin, end) of `rank`."""
    b, e = C.c_int(0), C.c_int(0)
    _check(_shard_range(int(nblocks), int(rank), int(world), C.byref(b), C.byref(e)))
    return b.value, e.value


def track_init(eph, iono, week, sec, xyz, trk):
    """allocateChannel()'s range / carrier-phase initialisation (reference gps.c:2199-2214); trk is updated in place."""
    eph = np.ascontiguousarray(eph, dtype=EPHEM_DTYPE)
    iono = np.ascontiguousarray(iono, dtype=IONO_DTYPE)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    assert trk.dtype == TRACK_DTYPE and trk.flags.c_contiguous
    _check(_track_init(_p(eph), _p(iono), int(week), float(sec), _p(xyz), _p(trk), len(trk)))
    return trk


def sat_visibility(eph, week, sec, xyz, elv_mask_deg=0.0):
    """checkSatVisibility() (reference gps.c:2142-2162) for one ephemeris: (visible, azel[2] in radians)."""
    eph = np.ascontiguousarray(eph, dtype=EPHEM_DTYPE)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    azel = np.zeros(2)
    return bool(_check(_sat_visibility(_p(eph), int(week), float(sec), _p(xyz), float(elv_mask_deg), _p(azel)))), azel


def refresh_batch(eph, iono, week, sec, xyz, trk, gain_x2=False, nthreads=0, out=None):
    """The per-block host refresh (reference gps.c:2731-2765) for len(xyz) blocks -> gpsiq_chan_t[nblocks][nchan].
    out: optional preallocated C-contiguous [len(xyz)][len(trk)] array (every field is written)."""
    eph = np.ascontiguousarray(eph, dtype=EPHEM_DTYPE)
    iono = np.ascontiguousarray(iono, dtype=IONO_DTYPE)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    assert trk.dtype == TRACK_DTYPE and trk.flags.c_contiguous
    if out is None:
        out = np.zeros((len(xyz), len(trk)), dtype=CHAN_DTYPE)
    assert out.dtype == CHAN_DTYPE and out.shape == (len(xyz), len(trk)) and out.flags.c_contiguous
    _check(_refresh_batch(_p(eph), _p(iono), int(week), float(sec), _p(xyz), len(xyz), len(trk), int(bool(gain_x2)),
                          _p(trk), _p(out), int(nthreads)))
    return out


def refresh_epochs(eph, iono, week, sec, xyz, trk_epochs, first_block, gain_x2=False, nthreads=0, out=None):
    """gpsiq_refresh_epochs: refresh_batch over several navigation-message epochs in one threaded pass.
    trk_epochs [nepochs][nchan] (TRACK_DTYPE): epoch e's word buffer and g0; first_block [nepochs]."""
    eph = np.ascontiguousarray(eph, dtype=EPHEM_DTYPE)
    iono = np.ascontiguousarray(iono, dtype=IONO_DTYPE)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    assert trk_epochs.dtype == TRACK_DTYPE and trk_epochs.flags.c_contiguous and trk_epochs.ndim == 2
    first = np.ascontiguousarray(first_block, dtype=np.int32)
    ne, nc = trk_epochs.shape
    assert len(first) == ne
    if out is None:
        out = np.empty((len(xyz), nc), dtype=CHAN_DTYPE)
    assert out.dtype == CHAN_DTYPE and out.shape == (len(xyz), nc) and out.flags.c_contiguous
    _check(_refresh_epochs(_p(eph), _p(iono), int(week), float(sec), _p(xyz), len(xyz), nc, int(bool(gain_x2)),
                           _p(trk_epochs), _p(first), ne, _p(out), int(nthreads)))
    return out


def refresh_epochs_quantized(eph, iono, week, sec, xyz, trk_epochs, first_block, fs, nsamp, gain_x2=False, nthreads=0, out=None):
    """gpsiq_refresh_epochs_quantized: refresh_epochs + quantize_blocks(carry0=None) in one pass -> QCHAN_DTYPE[nblocks][nchan]."""
    eph = np.ascontiguousarray(eph, dtype=EPHEM_DTYPE)
    iono = np.ascontiguousarray(iono, dtype=IONO_DTYPE)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    assert trk_epochs.dtype == TRACK_DTYPE and trk_epochs.flags.c_contiguous and trk_epochs.ndim == 2
    first = np.ascontiguousarray(first_block, dtype=np.int32)
    ne, nc = trk_epochs.shape
    assert len(first) == ne
    if out is None:
        out = np.empty((len(xyz), nc), dtype=QCHAN_DTYPE)
    assert out.dtype == QCHAN_DTYPE and out.shape == (len(xyz), nc) and out.flags.c_contiguous
    _check(_refresh_epochs_q(_p(eph), _p(iono), int(week), float(sec), _p(xyz), len(xyz), nc, int(bool(gain_x2)),
                             _p(trk_epochs), _p(first), ne, float(fs), int(nsamp), _p(out), int(nthreads)))
    return out


def llh_to_ecef(lat_rad, lon_rad, h):
    """llh2xyz() (reference gps.c:412-447): radians, metres -> ECEF metres."""
    llh = np.array([lat_rad, lon_rad, h], dtype=np.float64)
    xyz = np.zeros(3)
    _llh_to_ecef(_p(llh), _p(xyz))
    return xyz


def ecef_add_neu(llh_ref, neu, xyz):
    """xyz + ltcmat(llh_ref)^T * neu (reference gps.c:2354-2356, 2726-2728): a new array."""
    llh = np.ascontiguousarray(llh_ref, dtype=np.float64)
    d = np.ascontiguousarray(neu, dtype=np.float64)
    out = np.array(xyz, dtype=np.float64).copy()
    _ecef_add_neu(_p(llh), _p(d), _p(out))
    return out


def ecef_to_llh(xyz):
    """xyz2llh() (reference gps.c:361-410)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    llh = np.zeros(3)
    _ecef_to_llh(_p(xyz), _p(llh))
    return llh


def motion_read_csv(path, max_points=3000):
    """readUserMotion() (reference gps.c:2253-2277): -> xyz[n][3]; raises if the file cannot be opened."""
    xyz = np.zeros((max_points, 3), dtype=np.float64)
    n = _motion_read_csv(os.fsencode(path), _p(xyz), int(max_points))
    if n < 0:
        raise GpsiqError(n, _last_error().decode())
    return xyz[:n].copy()


def date_to_gps(year, month, day, hour=0, minute=0, second=0.0):
    """date2gps() (reference gps.c:315-337) -> (week, seconds of the week)."""
    w, sec = C.c_int(0), C.c_double(0.0)
    _date_to_gps(int(year), int(month), int(day), int(hour), int(minute), float(second), C.byref(w), C.byref(sec))
    return w.value, sec.value


def gps_to_date(week, sec):
    """gps2date() (reference gps.c:339-355) -> (year, month, day, hour, minute, second)."""
    v = [C.c_int(0) for _ in range(5)]
    s = C.c_double(0.0)
    _gps_to_date(int(week), float(sec), *[C.byref(x) for x in v], C.byref(s))
    return tuple(x.value for x in v) + (s.value,)


def nav_parity(source, nib=False):
    return int(_nav_parity(int(source) & 0xFFFFFFFF, int(bool(nib))))


def almanac_read_sem(path):
    """almanac_read_file() (reference almanac.c:73-184) -> (NAV_ALM_DTYPE[32], number of valid entries)."""
    alm = np.zeros(32, dtype=NAV_ALM_DTYPE)
    n = _almanac_read_sem(str(path).encode(), _p(alm))
    if n < 0:
        _check(n)
    return alm, n


def nav_subframes(eph, utc, alm=None):
    """eph2sbf(): -> uint32[53][10]"""
    eph = np.ascontiguousarray(eph, dtype=NAV_EPH_DTYPE)
    utc = np.ascontiguousarray(utc, dtype=NAV_UTC_DTYPE)
    sbf = np.zeros((53, 10), dtype=np.uint32)
    a = None if alm is None else np.ascontiguousarray(alm, dtype=NAV_ALM_DTYPE)
    assert a is None or len(a) == 32
    _check(_nav_subframes(_p(eph), _p(utc), None if a is None else _p(a), _p(sbf)))
    return sbf


def nav_message(sbf, week, sec, init, state):
    """generateNavMsg(): state (NAV_STATE_DTYPE scalar array of shape (1,)) is updated in place."""
    sbf = np.ascontiguousarray(sbf, dtype=np.uint32)
    assert sbf.shape == (53, 10) and state.dtype == NAV_STATE_DTYPE and state.size == 1
    _check(_nav_message(_p(sbf), int(week), float(sec), int(bool(init)), _p(state)))
    return state


def nav_roll(sbf, week, sec, states):
    """generateNavMsg(.., 0) for every channel in one call: sbf [nchan][53][10], states NAV_STATE_DTYPE[nchan] (in place)."""
    sbf = np.ascontiguousarray(sbf, dtype=np.uint32)
    assert sbf.ndim == 3 and sbf.shape[1:] == (53, 10) and states.dtype == NAV_STATE_DTYPE and len(states) == len(sbf) and states.flags.c_contiguous
    _check(_nav_roll(_p(sbf), len(sbf), int(week), float(sec), _p(states)))
    return states


def rinex_read(path, version=2):
    """readRinex2/readRinex3 -> (eph[13][32] RINEX_EPH_DTYPE, utc NAV_UTC_DTYPE, nsets).  nsets < 0:
    the reference's error codes (-1 open, -2 version, -3 file type)."""
    eph = np.zeros((13, 32), dtype=RINEX_EPH_DTYPE)
    utc = np.zeros(1, dtype=NAV_UTC_DTYPE)
    n = _rinex_read(os.fsencode(path), int(version), _p(eph), _p(utc))
    return eph, utc[0], n


def rinex_overwrite_time(eph, nsets, utc, week, sec):
    """The reference's -T option (gps.c:2534-2561): shift toc / toe / calendar time of every valid record so that the
    file serves the start time (week, sec); in place on eph[:nsets] and utc."""
    assert eph.dtype == RINEX_EPH_DTYPE and eph.flags.c_contiguous and utc.dtype == NAV_UTC_DTYPE
    _check(_rinex_overwrite_time(_p(eph), int(nsets), _p(utc), int(week), float(sec)))
    return eph, utc


def rinex_select(eph, nsets, week, sec):
    eph = np.ascontiguousarray(eph, dtype=RINEX_EPH_DTYPE)
    return int(_rinex_select(_p(eph), int(nsets), int(week), float(sec)))


def noise_sigma_for_cn0(cn0_dbhz, gain=1.0, fs=2.6e6):
    """Receiver-noise sigma (accumulator units) that puts a channel of this gain at cn0_dbhz dB-Hz at fs Hz."""
    return _noise_sigma_for_cn0(float(cn0_dbhz), float(gain), float(fs))


def composite_rms(gains, sigma=0.0):
    """Rms per component (I or Q) of channels with these gains plus noise of this sigma, in accumulator units."""
    g = np.ascontiguousarray(gains, dtype=np.float64).ravel()
    return _composite_rms(_p(g) if g.size else None, int(g.size), float(sigma))


def level_mult(rms_in, rms_out):
    """The Q16 multiplier of Context.set_level that takes rms_in to rms_out (include/gpsiq_rows.h, "Output level")."""
    return int(_level_mult(float(rms_in), float(rms_out)))


def packed_block_bytes(nsamp, bits):
    """gpsiq_packed_block_bytes: bytes of one packed block (include/gpsiq_rows.h, "Packed streams")."""
    return int(_packed_block_bytes(int(nsamp), int(bits)))


def cn0_estimate(sums, seg_len, fs):
    """gpsiq_cn0_estimate: (C/N0 in dB-Hz, its one-sigma in dB) of one channel from its full-length segments' sums (DESPREAD_SUM_DTYPE,
    any shape: every element is one segment)."""
    s = np.ascontiguousarray(sums, dtype=DESPREAD_SUM_DTYPE).ravel()
    cn0, one = _d(0.0), _d(0.0)
    _check(_cn0_estimate(_p(s) if s.size else None, int(s.size), int(seg_len), float(fs), C.byref(cn0), C.byref(one)))
    return cn0.value, one.value


def acquire_steps(fs, f0_hz, df_hz):
    """gpsiq_acquire_steps: (code_step, carr_step0, carr_step_inc) of a search at sample rate fs whose bins are f0_hz + d * df_hz."""
    cs, c0, ci = C.c_uint64(0), C.c_int64(0), C.c_int64(0)
    _check(_acquire_steps(float(fs), float(f0_hz), float(df_hz), C.byref(cs), C.byref(c0), C.byref(ci)))
    return int(cs.value), int(c0.value), int(ci.value)


def acquire_decide(power, guard):
    """gpsiq_acquire_decide on one satellite's grid power[ndopp][nshift]: (bin, shift, ratio of the best cell to the largest cell more
    than `guard` samples from its shift)."""
    g = np.ascontiguousarray(power, dtype=np.float64)
    assert g.ndim == 2
    d, s, r = _i(0), _i(0), _d(0.0)
    _check(_acquire_decide(_p(g) if g.size else None, int(g.shape[0]), int(g.shape[1]), int(guard), C.byref(d), C.byref(s), C.byref(r)))
    return d.value, s.value, r.value


def follow_gains(fs, fll_gain=0.25, pll_bn_hz=18.0, dll_bn_hz=5.0):
    """gpsiq_follow_gains: the follower's configuration (FOLLOW_CFG_DTYPE, one element) at sample rate fs.  The defaults are tuned for
    strong signals."""
    cfg = np.zeros(1, dtype=FOLLOW_CFG_DTYPE)
    _check(_follow_gains(float(fs), float(fll_gain), float(pll_bn_hz), float(dll_bn_hz), _p(cfg)))
    return cfg


def follow_start(prn, shift, dopp, code_step, carr_step0, carr_step_inc):
    """The follower's state (FOLLOW_STATE_DTYPE, one element per satellite) from acquisition peaks: satellite prn[k] found at sample
    shift[k] of bin dopp[k] of a search with the steps of acquire_steps.  The pull-in reaches |frequency error| < 250 Hz (beyond it
    lies a false lock 500 Hz off), so the search must use bins of 250 Hz or finer."""
    prn, shift, dopp = (np.atleast_1d(np.asarray(a)) for a in (prn, shift, dopp))
    st = np.zeros(len(prn), dtype=FOLLOW_STATE_DTYPE)
    st["prn"], st["sample"] = prn, shift
    st["code_step0"] = st["code_step"] = int(code_step)
    st["carr_step"] = st["carr_int"] = [int(carr_step0) + int(d) * int(carr_step_inc) for d in dopp]
    return st


def follow_bits(epochs, skip=0):
    """gpsiq_follow_bits on one satellite's records (FOLLOW_EPOCH_DTYPE [nepochs]): (offset of the bit edge in 0..19, int8 bits +1 / -1,
    0 for a zero sum).  The whole sequence may be negated (the polarity of a Costas loop)."""
    e = np.ascontiguousarray(epochs, dtype=FOLLOW_EPOCH_DTYPE).ravel()
    bits = np.zeros(max(len(e) // 20, 1), dtype=np.int8)
    off, nb = _i(0), _i(0)
    _check(_follow_bits(_p(e), int(e.size), int(skip), C.byref(off), _p(bits), int(bits.size), C.byref(nb)))
    return off.value, bits[:nb.value].copy()


def filter_span(nsamp, decim, phase=0):
    """gpsiq_filter_span: (outputs of a span of nsamp samples decimated by decim from input index phase, the phase its continuation
    starts at)."""
    nout, nxt = _i(0), _i(0)
    _check(_filter_span(int(nsamp), int(decim), int(phase), C.byref(nout), C.byref(nxt)))
    return nout.value, nxt.value


def filter_design(fs, cutoff_hz, ntaps, shift=14):
    """gpsiq_filter_design: int16 taps [ntaps] of a Hamming-windowed sinc low-pass with its -6 dB point at cutoff_hz, symmetric, their
    sum exactly 2**shift."""
    taps = np.zeros(max(int(ntaps), 1), dtype=np.int16)
    _check(_filter_design(float(fs), float(cutoff_hz), int(ntaps), int(shift), _p(taps)))
    return taps


def _u64_arg(v, what):
    v = int(v)
    if not 0 <= v < 2 ** 64:
        raise GpsiqError(-1, f"{what} {v} does not fit 64 unsigned bits")
    return v


def resample_span(nsamp, pos0, step):
    """gpsiq_resample_span: (outputs of a span of nsamp samples from position pos0 at `step` input samples an output, the position its
    continuation starts at); positions and steps in units of 2**-32 input sample."""
    nout, nxt = _u64(0), _u64(0)
    _check(_resample_span(_u64_arg(nsamp, "nsamp"), _u64_arg(pos0, "pos0"), _u64_arg(step, "step"), C.byref(nout), C.byref(nxt)))
    return int(nout.value), int(nxt.value)


def agc_mult(cfg, sumsq, count):
    """gpsiq_agc_mult: the gain rule -- the Q16 multiplier of a window whose ring holds `sumsq` as its sum of squares over `count`
    elements."""
    mult = C.c_uint32(0)
    _check(_agc_mult(C.byref(cfg) if cfg is not None else None, _u64_arg(sumsq, "sumsq"), _u64_arg(count, "count"), C.byref(mult)))
    return int(mult.value)


def agc_span(nsamp, window, fill=0):
    """gpsiq_agc_span: (windows a span of nsamp samples touches when `fill` samples of the window in progress lie before it, the fill it
    leaves)."""
    nwin, nxt = _u64(0), C.c_uint32(0)
    fill = int(fill)
    if not 0 <= fill < 2 ** 32:
        raise GpsiqError(-1, f"fill {fill} does not fit 32 unsigned bits")
    _check(_agc_span(_u64_arg(nsamp, "nsamp"), int(window), fill, C.byref(nwin), C.byref(nxt)))
    return int(nwin.value), int(nxt.value)


def notch_find(power, fs, ratio=8.0, max_lines=8):
    """gpsiq_notch_find: the lines of ONE group of a spectrum (uint64 [nfft]) -> (f_hz, excess_db, nlines): float arrays of the
    min(nlines, max_lines) strongest lines, strongest first, and the number of lines found before that cap."""
    power = np.ascontiguousarray(power, dtype=np.uint64)
    if power.ndim != 1:
        raise GpsiqError(-1, f"one group of a spectrum is a vector, not an array of shape {power.shape}")
    f, ex, n = np.zeros(8, np.float64), np.zeros(8, np.float64), _i(0)
    _check(_notch_find(_p(power), len(power), float(fs), float(ratio), int(max_lines), _p(f), _p(ex), C.byref(n)))
    keep = min(int(n.value), int(max_lines))
    return f[:keep].copy(), ex[:keep].copy(), int(n.value)


def notch_design(fs, f_hz, width_hz, ntaps, shift=12):
    """gpsiq_notch_design: int16 [ntaps, 2] (re, im) of a linear-phase notch at the frequencies f_hz (1..8 of them), each width_hz wide,
    over 2^shift."""
    f = np.ascontiguousarray(np.atleast_1d(f_hz), dtype=np.float64)
    taps = np.zeros((max(int(ntaps), 1), 2), dtype=np.int16)
    _check(_notch_design(float(fs), _p(f), len(f), float(width_hz), int(ntaps), int(shift), _p(taps)))
    return taps


def array_steer(pos, az_rad, el_rad):
    """gpsiq_array_steer: the phase advance, in cycles in [0, 1), of a plane wave from azimuth az_rad (from north towards east) and
    elevation el_rad at the elements at pos [nelem, 3] (east, north, up in wavelengths) -> float64 [nelem]."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise GpsiqError(-1, f"element positions are [nelem, 3] (east, north, up), not an array of shape {pos.shape}")
    out = np.zeros(max(len(pos), 1), dtype=np.float64)
    _check(_array_steer(_p(pos) if len(pos) else None, len(pos), float(az_rad), float(el_rad), _p(out)))
    return out[:len(pos)].copy()


def array_weights(cov, nsamp, steer=None, loading=0.0, shift=12):
    """gpsiq_array_weights: the combiner's weights int16 [nelem, 2] (re, im) over 2**shift from a covariance int64 [nelem, nelem, 2] of
    nsamp samples: power inversion with element 0 the reference (steer None), or minimum variance towards the steering phases `steer`
    (cycles, from array_steer); `loading` adds that fraction of the mean diagonal to the diagonal."""
    cov = np.ascontiguousarray(cov, dtype=np.int64)
    if cov.ndim != 3 or cov.shape[0] != cov.shape[1] or cov.shape[2] != 2:
        raise GpsiqError(-1, f"a covariance is [nelem, nelem, 2] (re, im), not an array of shape {cov.shape}")
    nelem = cov.shape[0]
    st = None
    if steer is not None:
        st = np.ascontiguousarray(steer, dtype=np.float64).ravel()
        if len(st) != nelem:
            raise GpsiqError(-1, f"{len(st)} steering phases for {nelem} elements")
    w = np.zeros((max(nelem, 1), 2), dtype=np.int16)
    _check(_array_weights(_p(cov) if cov.size else None, nelem, _u64_arg(nsamp, "nsamp"), None if st is None else _p(st), float(loading), int(shift),
                          _p(w)))
    return w[:nelem].copy()


def stap_weights(cov, nsamp, nelem, ntaps, steer=None, ref_tap=0, loading=0.0, shift=12):
    """gpsiq_stap_weights: the tapped combiner's weights int16 [nelem, ntaps, 2] (re, im) over 2**shift from a space-time covariance
    int64 [K, K, 2], K = nelem * ntaps, of nsamp samples: the constraint sits on the rows of tap ref_tap -- element 0 alone (steer
    None: power inversion) or the steering phases `steer` (cycles, from array_steer); `loading` as array_weights."""
    cov = np.ascontiguousarray(cov, dtype=np.int64)
    nelem, ntaps = int(nelem), int(ntaps)
    if cov.ndim != 3 or cov.shape[0] != cov.shape[1] or cov.shape[2] != 2 or cov.shape[0] != nelem * ntaps:
        raise GpsiqError(-1, f"a space-time covariance of {nelem} elements and {ntaps} taps is [{nelem * ntaps}, {nelem * ntaps}, 2], not {cov.shape}")
    st = None
    if steer is not None:
        st = np.ascontiguousarray(steer, dtype=np.float64).ravel()
        if len(st) != nelem:
            raise GpsiqError(-1, f"{len(st)} steering phases for {nelem} elements")
    w = np.zeros((max(nelem * ntaps, 1), 2), dtype=np.int16)
    _check(_stap_weights(_p(cov) if cov.size else None, nelem, ntaps, _u64_arg(nsamp, "nsamp"), None if st is None else _p(st), int(ref_tap),
                         float(loading), int(shift), _p(w)))
    return w[:nelem * ntaps].reshape(nelem, ntaps, 2).copy()


def stap_beam_weights(cov, nsamp, nelem, ntaps, steers, ref_tap=0, loading=0.0, shift=12):
    """gpsiq_stap_beam_weights: one set of stap_weights per row of `steers` (cycles, [nbeams, nelem], from array_steer) from the same
    space-time covariance -> int16 [nbeams, nelem, ntaps, 2] (re, im); beam b is stap_weights(..., steer=steers[b]) bit for bit."""
    cov = np.ascontiguousarray(cov, dtype=np.int64)
    nelem, ntaps = int(nelem), int(ntaps)
    if cov.ndim != 3 or cov.shape[0] != cov.shape[1] or cov.shape[2] != 2 or cov.shape[0] != nelem * ntaps:
        raise GpsiqError(-1, f"a space-time covariance of {nelem} elements and {ntaps} taps is [{nelem * ntaps}, {nelem * ntaps}, 2], not {cov.shape}")
    st = np.ascontiguousarray(steers, dtype=np.float64)
    if st.ndim != 2 or st.shape[1] != nelem:
        raise GpsiqError(-1, f"steering phases are [nbeams, {nelem}], not an array of shape {st.shape}")
    nbeams = st.shape[0]
    w = np.zeros((max(nbeams * nelem * ntaps, 1), 2), dtype=np.int16)
    _check(_stap_beam_weights(_p(cov) if cov.size else None, nelem, ntaps, _u64_arg(nsamp, "nsamp"), _p(st) if st.size else None, nbeams, int(ref_tap),
                              float(loading), int(shift), _p(w)))
    return w[:nbeams * nelem * ntaps].reshape(nbeams, nelem, ntaps, 2).copy()


def array_element(desc, phases):
    """The descriptor timeline of one array element: a copy of desc (CHAN_DTYPE [nblocks, nchan]) with phases[channel] (cycles) added
    to every row's carr_phase, modulo 1.  gpsiq_generate_batch reads carr_phase only in block 0 and where a slot is re-allocated, so
    this is the same timeline seen through the element's geometric phase."""
    out = np.array(desc, dtype=CHAN_DTYPE, copy=True)
    if out.ndim != 2:
        raise GpsiqError(-1, f"a descriptor timeline is [nblocks, nchan], not an array of shape {out.shape}")
    ph = np.ascontiguousarray(phases, dtype=np.float64).ravel()
    if len(ph) != out.shape[1]:
        raise GpsiqError(-1, f"{len(ph)} phases for {out.shape[1]} channels")
    cp = np.mod(out["carr_phase"] + ph[None, :], 1.0)
    cp[cp >= 1.0] = 0.0                                      # (a tiny negative sum rounds up to 1)
    out["carr_phase"] = cp
    return out


def resample_step(fs_in, fs_out, ppb=0.0):
    """gpsiq_resample_step: the step from a stream at fs_in to a receiver at fs_out whose clock runs ppb parts per billion fast."""
    step = _u64(0)
    _check(_resample_step(float(fs_in), float(fs_out), float(ppb), C.byref(step)))
    return int(step.value)


def resample_design(step, bandwidth=0.8, log2_phases=7, ntaps=16, shift=14):
    """gpsiq_resample_design: int16 taps [2**log2_phases + 1][ntaps] of a Hamming-windowed sinc at every phase, its cutoff at
    `bandwidth` of the lower of the two Nyquist rates, every row summing to 2**shift."""
    rows = (1 << min(max(int(log2_phases), 0), 8)) + 1
    taps = np.zeros((rows, max(int(ntaps), 1)), dtype=np.int16)
    _check(_resample_design(_u64_arg(step, "step"), float(bandwidth), int(log2_phases), int(ntaps), int(shift), _p(taps)))
    return taps


def spectrum_span(nsamp, nfft, hop=None, navg=1):
    """gpsiq_spectrum_span: (segments of nfft samples, hop apart, in a span of nsamp samples; whole groups of navg of them)."""
    nseg, ngroups = _i(0), _i(0)
    _check(_spectrum_span(int(nsamp), int(nfft), int(nfft if hop is None else hop), int(navg), C.byref(nseg), C.byref(ngroups)))
    return nseg.value, ngroups.value


def spectrum_min_shift(sample_size, nfft, window, navg):
    """gpsiq_spectrum_min_shift: the smallest shift at which the sum of navg segments cannot pass 2**64 - 1."""
    s = _spectrum_min_shift(int(sample_size), int(nfft), int(window), int(navg))
    if s < 0:
        _check(s)
    return s


def spectrum_scale(nfft, window, navg, shift, fs):
    """gpsiq_spectrum_scale: the factor that turns a cell of Context.spectrum() into stream units squared per Hz."""
    v = _d(0.0)
    _check(_spectrum_scale(int(nfft), int(window), int(navg), int(shift), float(fs), C.byref(v)))
    return v.value


def mix_tone(fs, f0_hz, f1_hz=None, sweep_s=0.0):
    """gpsiq_mix_tone: (step, rate, sweep_period) of a tone at f0_hz, or of a sawtooth sweep from f0_hz to f1_hz every sweep_s seconds."""
    step, rate, period = C.c_int64(0), C.c_int64(0), C.c_uint32(0)
    _check(_mix_tone(float(fs), float(f0_hz), float(f0_hz if f1_hz is None else f1_hz), float(sweep_s), C.byref(step), C.byref(rate), C.byref(period)))
    return step.value, rate.value, period.value


def mix_gain(amplitude, kind, shift):
    """gpsiq_mix_gain: the integer gain that gives a term the amplitude (stream units) behind a rounding shift."""
    g = C.c_int32(0)
    _check(_mix_gain(float(amplitude), int(kind), int(shift), C.byref(g)))
    return g.value


def mix_advance(terms, done):
    """gpsiq_mix_advance: the terms of a continuation `done` samples on, as a new list (the arguments stay as they are)."""
    arr = _mix_terms(terms)
    _check(_mix_advance(arr, len(terms), int(done)))
    out = []
    for k in range(len(terms)):
        t = MixTerm()
        C.memmove(C.byref(t), C.byref(arr, k * C.sizeof(MixTerm)), C.sizeof(MixTerm))
        out.append(t)
    return out


def noise_host(seed, sigma, block, nsamp):
    """The library's host twin of the receiver noise: int32 array [nsamp, 2] of (zI, zQ) for absolute block `block`."""
    out = np.zeros((int(nsamp), 2), dtype=np.int32)
    _check(_noise_host(int(seed) & (2**64 - 1), float(sigma), int(block) & (2**64 - 1), int(nsamp), _p(out)))
    return out


def generate_batch_multi(contexts, desc, nsamp, fs, sample_size, host_ptr=None, device_ptrs=None, carr_out=None):
    """gpsiq_generate_batch_multi: one call, one contiguous block range per context.  host_ptr: one host buffer
    for the whole timeline; device_ptrs: one device pointer per context (its own range); neither: a numpy array."""
    desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
    nb, nc = desc.shape
    handles = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    co = None if carr_out is None else _p(carr_out)
    out = None
    if device_ptrs is not None:
        dp = (C.c_void_p * len(contexts))(*[int(p) for p in device_ptrs])
        _check(_generate_batch_multi(handles, len(contexts), _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), None, dp, co))
        return None
    if host_ptr is None:
        out = np.zeros((nb, 2 * nsamp), dtype=elem_dtype(sample_size))
        host_ptr = out.ctypes.data
    _check(_generate_batch_multi(handles, len(contexts), _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), _vp(host_ptr), None, co))
    return out


class Context:
    """One libgpsiq context = one GPU."""

    def __init__(self, device=0):
        h = _vp()
        _check(_create(C.byref(h), int(device)))
        self._h = h
        self.device = device
        self.resident_nchan = 0          # channel slots of the set set_descriptors() made resident (despread()'s output shape)

    def close(self):
        if self._h:
            _destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_nco_mode(self, mode):
        """NCO_FIXED (default) or NCO_REFERENCE for generate_block / generate_batch."""
        _check(_set_nco_mode(self._h, int(mode)))

    def set_noise(self, seed, sigma, next_block=0):
        """Receiver noise of standard deviation sigma (accumulator units; 0 = off) from `seed`; next_block is the absolute
        block index the next drop-in call starts from (include/gpsiq.h, "receiver noise")."""
        st = NoiseSettings(int(seed) & (2**64 - 1), float(sigma), int(next_block) & (2**64 - 1))
        _check(_set_noise(self._h, C.byref(st)))

    def noise_off(self):
        _check(_set_noise(self._h, None))

    def noise_state(self):
        """(seed, sigma, next_block) of the context's receiver noise."""
        st = NoiseSettings()
        _check(_noise_state(self._h, C.byref(st)))
        return st.seed, st.sigma, st.next_block

    def set_level(self, mult, qmax):
        """Output level stage: out = clamp(floor((S + z) * mult / 65536 + 1/2), -qmax, qmax) in the kernels, in place of the
        wrapping store (include/gpsiq_rows.h, "Output level"); level_off() restores it."""
        st = LevelSettings(int(mult), int(qmax))
        _check(_set_level(self._h, C.byref(st)))

    def level_off(self):
        _check(_set_level(self._h, None))

    def set_patches(self, patches):
        patches = np.ascontiguousarray(patches, dtype=PATCH_DTYPE)
        _check(_set_patches(self._h, _p(patches) if len(patches) else None, len(patches)))

    # -- drop-in entry points (host buffers) --
    def generate_block(self, ch, nsamp, fs, sample_size, host_ptr=None):
        """One 0.1 s block, the call that replaces gps.c:2767-2846.  host_ptr: optional
        caller-owned host buffer of 2*nsamp elements (e.g. a page-locked fifo buffer)."""
        ch = np.ascontiguousarray(ch, dtype=CHAN_DTYPE)
        carr = np.zeros(len(ch), dtype=np.float64)
        if host_ptr is not None:
            _check(_generate_block(self._h, _p(ch), len(ch), int(nsamp), float(fs), int(sample_size), _vp(host_ptr), _p(carr)))
            return None, carr
        out = np.zeros(2 * nsamp, dtype=elem_dtype(sample_size))
        _check(_generate_block(self._h, _p(ch), len(ch), int(nsamp), float(fs), int(sample_size), _p(out), _p(carr)))
        return out, carr

    def generate_block_async(self, ch, nsamp, fs, sample_size, host_ptr):
        """gpsiq_generate_block_async: queue one block into the page-locked buffer at host_ptr; returns the carrier
        phases to hand back in (final at once).  The samples are there after wait()."""
        ch = np.ascontiguousarray(ch, dtype=CHAN_DTYPE)
        carr = np.zeros(len(ch), dtype=np.float64)
        _check(_generate_block_async(self._h, _p(ch), len(ch), int(nsamp), float(fs), int(sample_size), _vp(host_ptr), _p(carr)))
        return carr

    def wait(self):
        _check(_wait(self._h))

    def generate_batch(self, desc, nsamp, fs, sample_size, device_ptr=None, host_ptr=None, carr_out=None):
        """carr_out: optional float64[nchan] array that receives the carrier phase after the
        last block (hand it back as block 0's carr_phase of the next batch to continue exactly).
        desc: a CHAN_DTYPE array [nblocks][nchan] (pageable or page-locked: a view is passed as it is), or a tuple
        (pointer, nblocks, nchan) for gpsiq_chan_t rows that lie in device or page-locked memory."""
        if isinstance(desc, tuple):
            dp, nb, nc = _vp(desc[0]), int(desc[1]), int(desc[2])
        else:
            desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
            nb, nc = desc.shape
            dp = _p(desc)
        co = None if carr_out is None else _p(carr_out)
        if host_ptr is not None:      # caller-owned host buffer (e.g. pinned), nb*2*nsamp elements
            _check(_generate_batch(self._h, dp, nb, nc, int(nsamp), float(fs), int(sample_size), _vp(host_ptr), 0, co))
            return None
        if device_ptr is not None:
            _check(_generate_batch(self._h, dp, nb, nc, int(nsamp), float(fs), int(sample_size), _vp(device_ptr), 1, co))
            return None
        out = np.zeros((nb, 2 * nsamp), dtype=elem_dtype(sample_size))
        _check(_generate_batch(self._h, dp, nb, nc, int(nsamp), float(fs), int(sample_size), _p(out), 0, co))
        return out

    def device_eval_host_ms(self):
        """Host time the last device-evaluated batch spent on descriptors (pack of pageable rows, repair, the host walker's share)."""
        return float(_device_eval_host_ms(self._h))

    def generate_quantized(self, q, nsamp, sample_size, device_ptr=None, host_ptr=None):
        """One shard of a time-sharded run: a slice of quantize_blocks()' output -> IQ elements."""
        q = np.ascontiguousarray(q, dtype=QCHAN_DTYPE)
        nb, nc = q.shape
        if host_ptr is not None:
            _check(_generate_quantized(self._h, _p(q), nb, nc, int(nsamp), int(sample_size), _vp(host_ptr), 0))
            return None
        if device_ptr is not None:
            _check(_generate_quantized(self._h, _p(q), nb, nc, int(nsamp), int(sample_size), _vp(device_ptr), 1))
            return None
        out = np.zeros((nb, 2 * nsamp), dtype=elem_dtype(sample_size))
        _check(_generate_quantized(self._h, _p(q), nb, nc, int(nsamp), int(sample_size), _p(out), 0))
        return out

    # -- resident-descriptor path (device buffers) --
    def generate_seeded(self, desc, nsamp, fs, sample_size, carr_start, device_ptr=None, host_ptr=None):
        """gpsiq_generate_seeded: GPSIQ_NCO_REFERENCE render of blocks whose start states are known (rows of reference_chain)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        nb, nc = desc.shape
        st = np.ascontiguousarray(carr_start, dtype=np.float64)
        assert st.shape == (nb, nc)
        if device_ptr is not None:
            _check(_generate_seeded(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), _p(st), _vp(device_ptr), 1))
            return None
        out = None
        if host_ptr is None:
            out = np.zeros((nb, 2 * nsamp), dtype=elem_dtype(sample_size))
            host_ptr = out.ctypes.data
        _check(_generate_seeded(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), _p(st), _vp(host_ptr), 0))
        return out

    def set_descriptors(self, q):
        q = np.ascontiguousarray(q, dtype=QCHAN_DTYPE)
        nb, nc = q.shape
        _check(_set_descriptors(self._h, _p(q), nb, nc))
        self.resident_nchan = nc

    def launch(self, block0, nblocks, nsamp, sample_size, device_ptr, block_stride, stream=None, variant=0):
        _check(_launch(self._h, int(block0), int(nblocks), int(nsamp), int(sample_size), _vp(device_ptr),
                       int(block_stride), _vp(stream or 0), int(variant)))

    def despread(self, block0, nblocks, nsamp, sample_size, device_ptr, block_stride, seg_len, clip=0, stream=None, stats=True, nchan=None):
        """gpsiq_despread: correlate the device stream at device_ptr (laid out as launch() writes it) with the replica of every
        active channel of the resident blocks [block0, block0 + nblocks) -> (sums DESPREAD_SUM_DTYPE [nblocks][nchan][nseg],
        prn uint8 [nblocks][nchan], stats BLOCK_STATS_DTYPE [nblocks] or None, kernel milliseconds).  Slots are in device order: a
        block's active channels counted from 0.  nchan: the resident set's channel slots where another call than set_descriptors()
        made it resident."""
        nc = int(nchan or self.resident_nchan)
        nseg = -(-int(nsamp) // int(seg_len)) if seg_len > 0 else 0
        sums = np.zeros((int(nblocks), nc, max(nseg, 0)), dtype=DESPREAD_SUM_DTYPE)
        prn = np.zeros((int(nblocks), nc), dtype=np.uint8)
        st = np.zeros(int(nblocks), dtype=BLOCK_STATS_DTYPE) if stats else None
        ms = C.c_float(0.0)
        _check(_despread(self._h, int(block0), int(nblocks), int(nsamp), int(sample_size), _vp(device_ptr), int(block_stride), _vp(stream or 0),
                         int(seg_len), int(clip), _p(sums), _p(prn), None if st is None else _p(st), C.byref(ms)))
        return sums, prn, st, float(ms.value)

    def despread_last_plan(self):
        """What the last despread() took: (kernel name or None, channel slots of the row kernel, grid, rows per wave)."""
        out = np.zeros(4, dtype=np.int32)
        _check(_despread_last_plan(self._h, _p(out)))
        return {0: "generic", 1: "rows"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def pack(self, nblocks, nsamp, sample_size, device_ptr, src_stride, bits, dst_device_ptr, dst_stride, stream=None):
        """gpsiq_pack: the device stream at device_ptr (laid out as launch() writes it) packed to `bits` (4 or 2) per component at
        dst_device_ptr -> (elements the packer had to clamp, kernel milliseconds)."""
        clipped, ms = C.c_uint64(0), C.c_float(0.0)
        _check(_pack(self._h, int(nblocks), int(nsamp), int(sample_size), _vp(device_ptr), int(src_stride), int(bits), _vp(dst_device_ptr),
                     int(dst_stride), _vp(stream or 0), C.byref(clipped), C.byref(ms)))
        return int(clipped.value), float(ms.value)

    def unpack(self, nblocks, nsamp, bits, device_ptr, src_stride, sample_size, dst_device_ptr, dst_stride, stream=None):
        """gpsiq_unpack: the packed device stream at device_ptr back into int8 / int16 elements at dst_device_ptr -> kernel milliseconds."""
        ms = C.c_float(0.0)
        _check(_unpack(self._h, int(nblocks), int(nsamp), int(bits), _vp(device_ptr), int(src_stride), int(sample_size), _vp(dst_device_ptr),
                       int(dst_stride), _vp(stream or 0), C.byref(ms)))
        return float(ms.value)

    def generate_batch_packed(self, desc, nsamp, fs, bits, host_ptr=None, block_stride=None, carr_out=None):
        """gpsiq_generate_batch_packed: the run-ahead call with packed blocks in host memory (the output level must be on with a
        qmax inside the format).  Returns uint8 [nblocks][packed_block_bytes], or None when host_ptr names the caller's buffer
        (pageable or page-locked; block_stride bytes between blocks, default: back to back)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        nb, nc = desc.shape
        plen = packed_block_bytes(nsamp, bits)
        stride = plen if block_stride is None else int(block_stride)
        co = None if carr_out is None else _p(carr_out)
        if host_ptr is not None:
            _check(_generate_batch_packed(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(bits), _vp(host_ptr), stride, co))
            return None
        out = np.zeros((nb, stride), dtype=np.uint8)
        _check(_generate_batch_packed(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(bits), _p(out), stride, co))
        return out[:, :plen]

    def acquire(self, nsamp, sample_size, device_ptr, prn, code_step, carr_step0, carr_step_inc, ndopp, nshift, ncoh, nnoncoh=1, hop=None,
                stream=None, power=True, corr=False):
        """gpsiq_acquire: search the nsamp complex samples at device_ptr for the satellites `prn` over ndopp bins and nshift shifts ->
        (peaks ACQ_PEAK_DTYPE [nprn][ndopp], power float64 [nprn][ndopp][nshift] or None, corr DESPREAD_SUM_DTYPE
        [nprn][ndopp][nnoncoh][nshift] or None, kernel milliseconds).  hop: samples between dwells (default ncoh)."""
        prn = np.ascontiguousarray(prn, dtype=np.uint8).ravel()
        hop = int(ncoh if hop is None else hop)
        shape = (len(prn), max(int(ndopp), 0))
        peaks = np.zeros(shape, dtype=ACQ_PEAK_DTYPE)
        pw = np.zeros(shape + (max(int(nshift), 0),), dtype=np.float64) if power else None
        cr = np.zeros(shape + (max(int(nnoncoh), 0), max(int(nshift), 0)), dtype=DESPREAD_SUM_DTYPE) if corr else None
        ms = C.c_float(0.0)
        _check(_acquire(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(stream or 0), _p(prn) if len(prn) else None, len(prn),
                        int(code_step), int(carr_step0), int(carr_step_inc), int(ndopp), int(nshift), int(ncoh), int(nnoncoh), hop, _p(peaks),
                        None if pw is None else _p(pw), None if cr is None else _p(cr), C.byref(ms)))
        return peaks, pw, cr, float(ms.value)

    def acquire_last_plan(self):
        """What the last acquire() took: (kernel name or None, bytes of digit planes, workgroups of the main kernel, k-steps,
        milliseconds of stage one, milliseconds of the rest)."""
        out = (C.c_longlong * 4)()
        ms = (C.c_float * 2)()
        _check(_acquire_last_plan(self._h, out, ms))
        return {0: "generic", 1: "mfma"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3]), float(ms[0]), float(ms[1])

    def follow(self, nsamp, sample_size, device_ptr, cfg, states, max_epochs, stream=None):
        """gpsiq_follow: follow the satellites of `states` (FOLLOW_STATE_DTYPE, from follow_start or an earlier call) through the nsamp
        complex samples at device_ptr with the configuration cfg (follow_gains) -> (records FOLLOW_EPOCH_DTYPE [nprn][max_epochs], of
        which the first nepochs[p] are written, nepochs int32 [nprn], the states to continue from, kernel milliseconds)."""
        cfg = np.ascontiguousarray(cfg, dtype=FOLLOW_CFG_DTYPE).ravel()
        assert cfg.size == 1
        st = np.array(states, dtype=FOLLOW_STATE_DTYPE, copy=True, ndmin=1).ravel()
        ep = np.zeros((len(st), max(int(max_epochs), 0)), dtype=FOLLOW_EPOCH_DTYPE)
        ne = np.zeros(len(st), dtype=np.int32)
        ms = C.c_float(0.0)
        _check(_follow(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(stream or 0), _p(cfg), _p(st) if len(st) else None, len(st),
                       _p(ep) if ep.size else None, int(max_epochs), _p(ne) if len(st) else None, C.byref(ms)))
        return ep, ne, st, float(ms.value)

    def follow_last_plan(self):
        """What the last follow() took: (workgroups of a launch or None, epochs a launch does per satellite at most, launches, bytes of
        records on the device)."""
        out = (C.c_longlong * 4)()
        _check(_follow_last_plan(self._h, out))
        return (None if out[0] < 0 else int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def filter(self, nsamp, sample_size, device_ptr, taps, shift, decim, phase, out_sample_size, dst_device_ptr, head_ptr=None, stream=None):
        """gpsiq_filter: the nsamp complex samples at device_ptr through the FIR `taps` (int16, host), rounded by `shift`, decimated by
        `decim` from input index `phase`, clamped into out_sample_size at dst_device_ptr; head_ptr: the ntaps - 1 samples before the span
        (None: zeros) -> (outputs written, elements the clamp changed, kernel milliseconds)."""
        taps = np.ascontiguousarray(taps, dtype=np.int16).ravel()
        nout, clipped, ms = _i(0), C.c_uint64(0), C.c_float(0.0)
        _check(_filter(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(head_ptr or 0), _p(taps) if len(taps) else None, len(taps), int(shift),
                       int(decim), int(phase), int(out_sample_size), _vp(dst_device_ptr), _vp(stream or 0), C.byref(nout), C.byref(clipped), C.byref(ms)))
        return nout.value, int(clipped.value), float(ms.value)

    def cfilter(self, nsamp, sample_size, device_ptr, taps, shift, decim, phase, out_sample_size, dst_device_ptr, head_ptr=None, stream=None):
        """gpsiq_cfilter: gpsiq_filter with complex taps ([n, 2] int16 (re, im), or CTap: ctaps()) -> (outputs written, elements the clamp
        changed, kernel milliseconds), as filter()."""
        taps = ctaps(taps)
        nout, clipped, ms = _i(0), C.c_uint64(0), C.c_float(0.0)
        _check(_cfilter(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(head_ptr or 0), _p(taps) if len(taps) else None, len(taps), int(shift),
                        int(decim), int(phase), int(out_sample_size), _vp(dst_device_ptr), _vp(stream or 0), C.byref(nout), C.byref(clipped), C.byref(ms)))
        return nout.value, int(clipped.value), float(ms.value)

    def cfilter_last_plan(self):
        """What the last cfilter() took: (kernel name or None, grid, outputs of a workgroup's run, k-steps of a tile)."""
        out = (C.c_long * 4)()
        _check(_cfilter_last_plan(self._h, out))
        return {0: "generic", 1: "mfma", 2: "mfma16"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def array_cov(self, ptrs, nsamp, sample_size, stream=None):
        """gpsiq_array_cov: the exact covariance of the streams at `ptrs` (device or page-locked addresses, one per element), nsamp
        complex samples each -> (int64 [nelem, nelem, 2] (re, im) of sum x_a conj(x_b), kernel milliseconds)."""
        ptrs = [int(p or 0) for p in ptrs]
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        cov = np.zeros((len(ptrs), len(ptrs), 2), dtype=np.int64)
        ms = C.c_float(0.0)
        _check(_array_cov(self._h, len(ptrs), arr, int(nsamp), int(sample_size), _vp(stream or 0), _p(cov) if cov.size else None, C.byref(ms)))
        return cov, float(ms.value)

    def array_combine(self, ptrs, nsamp, sample_size, weights, shift, out_sample_size, dst_device_ptr, stream=None):
        """gpsiq_array_combine: sum over the elements of weights[e] * stream e ([nelem, 2] int16 (re, im), or CTap: ctaps()), rounded by
        `shift`, clamped into out_sample_size at dst_device_ptr -> (elements the clamp changed, kernel milliseconds)."""
        ptrs = [int(p or 0) for p in ptrs]
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        w = ctaps(weights)
        if len(w) != len(ptrs):
            raise GpsiqError(-1, f"{len(w)} weights for {len(ptrs)} elements")
        clipped, ms = C.c_uint64(0), C.c_float(0.0)
        _check(_array_combine(self._h, len(ptrs), arr, int(nsamp), int(sample_size), _p(w) if len(w) else None, int(shift), int(out_sample_size),
                              _vp(dst_device_ptr), _vp(stream or 0), C.byref(clipped), C.byref(ms)))
        return int(clipped.value), float(ms.value)

    def array_last_plan(self):
        """What the last array_cov() / array_combine() took: (kernel name or None, grid, run of a workgroup or samples of a slot, elements)."""
        out = (C.c_long * 4)()
        _check(_array_last_plan(self._h, out))
        return {0: "generic", 1: "mfma", 2: "combine"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    @staticmethod
    def _stap_pointers(ptrs, heads):
        ptrs = [int(p or 0) for p in ptrs]
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        if heads is None:
            return ptrs, arr, None
        heads = [int(h or 0) for h in heads]
        if len(heads) != len(ptrs):
            raise GpsiqError(-1, f"{len(heads)} heads for {len(ptrs)} elements")
        return ptrs, arr, (C.c_void_p * max(len(heads), 1))(*heads)

    def stap_cov(self, ptrs, nsamp, sample_size, ntaps, heads=None, stream=None):
        """gpsiq_stap_cov: the exact covariance of the rows z[e * ntaps + t](n) = x_e(n - t) of the streams at `ptrs` (device or
        page-locked addresses, one per element), nsamp complex samples each; heads: None, or per element the address of the ntaps - 1
        samples before the span (None or 0: zeros) -> (int64 [K, K, 2] (re, im), K = len(ptrs) * ntaps, kernel milliseconds)."""
        ptrs, arr, harr = self._stap_pointers(ptrs, heads)
        rows = len(ptrs) * max(int(ntaps), 0)
        cov = np.zeros((rows, rows, 2), dtype=np.int64)
        ms = C.c_float(0.0)
        _check(_stap_cov(self._h, len(ptrs), arr, harr, int(nsamp), int(sample_size), int(ntaps), _vp(stream or 0),
                         _p(cov) if cov.size else None, C.byref(ms)))
        return cov, float(ms.value)

    def stap_combine(self, ptrs, nsamp, sample_size, weights, shift, out_sample_size, dst_device_ptr, heads=None, stream=None):
        """gpsiq_stap_combine: sum over elements and taps of weights[e][t] * x_e(n - t) (int16 [nelem, ntaps, 2] (re, im)), rounded by
        `shift`, clamped into out_sample_size at dst_device_ptr; heads as stap_cov -> (elements the clamp changed, kernel milliseconds)."""
        ptrs, arr, harr = self._stap_pointers(ptrs, heads)
        w = np.asarray(weights)
        if w.ndim != 3 or w.shape[0] != len(ptrs) or w.shape[2] != 2:
            raise GpsiqError(-1, f"tapped weights are [nelem, ntaps, 2] (re, im) for {len(ptrs)} elements, not an array of shape {w.shape}")
        ntaps = w.shape[1]
        w = ctaps(w.reshape(-1, 2))
        clipped, ms = C.c_uint64(0), C.c_float(0.0)
        _check(_stap_combine(self._h, len(ptrs), arr, harr, int(nsamp), int(sample_size), _p(w) if len(w) else None, int(ntaps), int(shift),
                             int(out_sample_size), _vp(dst_device_ptr), _vp(stream or 0), C.byref(clipped), C.byref(ms)))
        return int(clipped.value), float(ms.value)

    def stap_last_plan(self):
        """What the last stap_cov() / stap_combine() took: (kernel name or None, grid, run of a workgroup or samples of a slot, elements,
        taps)."""
        out = (C.c_long * 5)()
        _check(_stap_last_plan(self._h, out))
        return {0: "generic", 1: "mfma", 2: "combine"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3]), int(out[4])

    def stap_beams(self, ptrs, nsamp, sample_size, weights, shift, out_sample_size, dst_ptrs, heads=None, stream=None):
        """gpsiq_stap_beams: len(dst_ptrs) beams of the same element streams in one pass; beam b is stap_combine with weights[b] (int16
        [nbeams, nelem, ntaps, 2] (re, im)) written at dst_ptrs[b]; heads as stap_cov -> (elements the clamp changed per beam, uint64
        [nbeams], kernel milliseconds)."""
        ptrs, arr, harr = self._stap_pointers(ptrs, heads)
        w = np.asarray(weights)
        dsts = [int(d or 0) for d in dst_ptrs]
        if w.ndim != 4 or w.shape[0] != len(dsts) or w.shape[1] != len(ptrs) or w.shape[3] != 2:
            raise GpsiqError(-1, f"beam weights are [nbeams, nelem, ntaps, 2] (re, im) for {len(dsts)} beams of {len(ptrs)} elements, not an array of "
                                 f"shape {w.shape}")
        ntaps = w.shape[2]
        w = ctaps(w.reshape(-1, 2))
        darr = (C.c_void_p * max(len(dsts), 1))(*dsts)
        clipped = np.zeros(max(len(dsts), 1), dtype=np.uint64)
        ms = C.c_float(0.0)
        _check(_stap_beams(self._h, len(ptrs), arr, harr, int(nsamp), int(sample_size), _p(w) if len(w) else None, int(ntaps), len(dsts), int(shift),
                           int(out_sample_size), darr, _vp(stream or 0), _p(clipped), C.byref(ms)))
        return clipped[:len(dsts)].copy(), float(ms.value)

    def stap_beams_last_plan(self):
        """What the last stap_beams() took: (kernel name or None, grid, samples of a workgroup's run, elements, taps, beams, the taps an
        element is padded to in the matrix kernel's operand)."""
        out = (C.c_long * 7)()
        _check(_stap_beams_last_plan(self._h, out))
        return ({0: "generic", 1: "mfma"}.get(int(out[0])),) + tuple(int(v) for v in out[1:])

    def generate_batch_filtered(self, desc, nsamp, fs, sample_size, taps, shift, decim, out_sample_size, host_ptr=None, block_stride=None,
                                carr_out=None):
        """gpsiq_generate_batch_filtered: the run-ahead call rendered at sample_size, filtered and decimated on the device, with blocks
        of nsamp / decim samples of out_sample_size in host memory.  Returns (int8 / int16 [nblocks][2 * nsamp / decim], elements the
        clamp changed), the array None when host_ptr names the caller's buffer (pageable or page-locked; block_stride bytes between
        blocks, default: back to back)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        taps = np.ascontiguousarray(taps, dtype=np.int16).ravel()
        nb, nc = desc.shape
        rlen = 2 * (int(nsamp) // max(int(decim), 1)) * int(out_sample_size)
        stride = rlen if block_stride is None else int(block_stride)
        co = None if carr_out is None else _p(carr_out)
        clipped = C.c_uint64(0)
        out = None if host_ptr is not None else np.zeros((nb, stride), dtype=np.uint8)
        _check(_generate_batch_filtered(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), _p(taps) if len(taps) else None, len(taps),
                                        int(shift), int(decim), int(out_sample_size), _vp(host_ptr) if out is None else _p(out), stride,
                                        C.byref(clipped), co))
        if out is None:
            return None, int(clipped.value)
        return np.ascontiguousarray(out[:, :rlen]).view(np.int8 if int(out_sample_size) == 1 else np.int16), int(clipped.value)

    def filter_last_plan(self):
        """What the last filter() / generate_batch_filtered() took: (kernel name or None, grid, outputs of a workgroup's run, pieces)."""
        out = (C.c_long * 4)()
        _check(_filter_last_plan(self._h, out))
        return {0: "generic", 1: "mfma"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def spectrum(self, nsamp, sample_size, device_ptr, nfft, hop=None, window=1, navg=None, shift=None, stream=None, out=None):
        """gpsiq_spectrum: the exact integer power spectrum of the nsamp complex samples at device_ptr -> uint64 [ngroups][nfft].  hop
        defaults to nfft, navg to all segments in one group, shift to spectrum_min_shift.  out: a C-contiguous uint64 array the call
        writes instead of a fresh one (the caller's to size).  The kernels' device time of the last call is self.spectrum_ms."""
        hop = int(nfft) if hop is None else int(hop)
        if navg is None:
            navg = max(spectrum_span(nsamp, nfft, hop, 1)[0], 1)
        if shift is None:
            shift = spectrum_min_shift(sample_size, nfft, window, navg)
        if out is None:
            try:
                groups = spectrum_span(nsamp, nfft, hop, navg)[1]
            except GpsiqError:
                groups = 0                                            # the call itself refuses what the span arithmetic refuses
            out = np.zeros((max(groups, 1), max(int(nfft), 1)), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous
        ng, ms = _i(0), C.c_float(0.0)
        _check(_spectrum(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(stream or 0), int(nfft), hop, int(window), int(navg), int(shift),
                         _p(out), C.byref(ng), C.byref(ms)))
        self.spectrum_ms = float(ms.value)
        return out.reshape(-1, int(nfft))[:ng.value]

    def spectrum_last_plan(self):
        """What the last spectrum() took: (kernel name or None, grid, segments of a unit or a pass, groups)."""
        out = (C.c_longlong * 4)()
        _check(_spectrum_last_plan(self._h, out))
        return {0: "generic", 1: "mfma"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def mix(self, nsamp, m0, terms, shift, qmax, out_sample_size, dst_device_ptr, stream=None):
        """gpsiq_mix: the sum of the MixTerm list `terms` over nsamp samples from absolute index m0, rounded by `shift`, clamped to
        +-qmax into out_sample_size at dst_device_ptr (which may be a stream term's own source: in place) -> (elements the clamp
        changed, kernel milliseconds)."""
        arr = _mix_terms(terms)
        clipped, ms = C.c_uint64(0), C.c_float(0.0)
        _check(_mix(self._h, int(nsamp), int(m0) % 2 ** 64, arr, len(terms), int(shift), int(qmax), int(out_sample_size), _vp(dst_device_ptr),
                    _vp(stream or 0), C.byref(clipped), C.byref(ms)))
        return int(clipped.value), float(ms.value)

    def generate_batch_mixed(self, desc, nsamp, fs, sample_size, base_gain, tones, shift, qmax, m0=0, host_ptr=None, block_stride=None,
                             carr_out=None):
        """gpsiq_generate_batch_mixed: the run-ahead call with base_gain times the rendered stream plus the MixTerm tones, rounded by
        `shift` and clamped to +-qmax, in host memory.  Returns (int8 / int16 [nblocks][2 * nsamp], elements the clamp changed), the
        array None when host_ptr names the caller's buffer (pageable or page-locked; block_stride bytes between blocks, default: back
        to back)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        nb, nc = desc.shape
        rlen = 2 * int(nsamp) * int(sample_size)
        stride = rlen if block_stride is None else int(block_stride)
        co = None if carr_out is None else _p(carr_out)
        clipped = C.c_uint64(0)
        out = None if host_ptr is not None else np.zeros((nb, stride), dtype=np.uint8)
        arr = _mix_terms(tones)
        _check(_generate_batch_mixed(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), int(base_gain), arr, len(tones),
                                     int(m0) % 2 ** 64, int(shift), int(qmax), _vp(host_ptr) if out is None else _p(out), stride, C.byref(clipped), co))
        if out is None:
            return None, int(clipped.value)
        return np.ascontiguousarray(out[:, :rlen]).view(np.int8 if int(sample_size) == 1 else np.int16), int(clipped.value)

    def mix_last_plan(self):
        """What the last mix() / generate_batch_mixed() took: (kernel name or None, grid, units of the launch, pieces)."""
        out = (C.c_longlong * 4)()
        _check(_mix_last_plan(self._h, out))
        return {0: "generic", 1: "rows"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def resample(self, nsamp, sample_size, device_ptr, taps, log2_phases, shift, interp, step, pos0, out_sample_size, dst_device_ptr, head_ptr=None,
                 stream=None):
        """gpsiq_resample: the nsamp complex samples at device_ptr resampled at positions pos0 + j * step (2**-32 input sample) through the
        table `taps` (int16 [2**log2_phases + 1][ntaps], host), rounded by `shift`, clamped into out_sample_size at dst_device_ptr;
        head_ptr: the ntaps - 1 samples before the span (None: zeros) -> (outputs written, next position, elements the clamp changed,
        kernel milliseconds)."""
        taps = np.ascontiguousarray(taps, dtype=np.int16)
        ntaps = taps.shape[-1] if taps.ndim == 2 else 0
        nout, nxt, clipped, ms = _u64(0), _u64(0), _u64(0), C.c_float(0.0)
        _check(_resample(self._h, int(nsamp), int(sample_size), _vp(device_ptr), _vp(head_ptr or 0), _p(taps) if taps.size else None, int(log2_phases),
                         int(ntaps), int(shift), int(interp), _u64_arg(step, "step"), _u64_arg(pos0, "pos0"), int(out_sample_size),
                         _vp(dst_device_ptr), _vp(stream or 0), C.byref(nout), C.byref(nxt), C.byref(clipped), C.byref(ms)))
        return int(nout.value), int(nxt.value), int(clipped.value), float(ms.value)

    def generate_batch_resampled(self, desc, nsamp, fs, sample_size, taps, log2_phases, shift, interp, step, pos0, out_sample_size, host_ptr=None,
                                 capacity=None, carr_out=None):
        """gpsiq_generate_batch_resampled: the run-ahead call rendered at sample_size and resampled on the device into ONE stream of
        out_sample_size in host memory.  Returns (int8 / int16 [nout][2], elements the clamp changed), with the count in the array's
        place when host_ptr names the caller's buffer of `capacity` samples (pageable or page-locked)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        taps = np.ascontiguousarray(taps, dtype=np.int16)
        ntaps = taps.shape[-1] if taps.ndim == 2 else 0
        nb, nc = desc.shape
        co = None if carr_out is None else _p(carr_out)
        nout, clipped = _u64(0), _u64(0)
        out = None
        if host_ptr is None:
            capacity = resample_span(nb * int(nsamp), pos0, step)[0] if capacity is None else int(capacity)
            out = np.zeros((max(capacity, 1), 2), dtype=np.int8 if int(out_sample_size) == 1 else np.int16)
        _check(_generate_batch_resampled(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), _p(taps) if taps.size else None,
                                         int(log2_phases), int(ntaps), int(shift), int(interp), _u64_arg(step, "step"), _u64_arg(pos0, "pos0"),
                                         int(out_sample_size), _vp(host_ptr) if out is None else _p(out), _u64_arg(capacity, "capacity"), C.byref(nout),
                                         C.byref(clipped), co))
        if out is None:
            return int(nout.value), int(clipped.value)
        return out[:int(nout.value)], int(clipped.value)

    def resample_last_plan(self):
        """What the last resample() / generate_batch_resampled() took: (kernel name or None, grid, outputs of a unit, pieces)."""
        out = (C.c_longlong * 4)()
        _check(_resample_last_plan(self._h, out))
        return {0: "generic", 1: "rows"}.get(int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def agc(self, nsamp, sample_size, device_ptr, cfg, out_sample_size, dst_device_ptr, state=None, stream=None):
        """gpsiq_agc: the nsamp complex samples at device_ptr through the blanker, the windowed gain and the clamp of `cfg` (AgcCfg) into
        out_sample_size at dst_device_ptr.  state: an AgcState, updated in place (None: a fresh stream, nothing returned) -> (elements
        the clamp changed, samples blanked, uint32 multipliers of the windows touched, kernel milliseconds)."""
        fill = 0 if state is None else int(state.fill)
        window = int(cfg.window) if cfg is not None else 0
        nwin = (fill + int(nsamp) + window - 1) // window if window > 0 and int(nsamp) > 0 else 0
        mults = np.zeros(max(nwin, 1), dtype=np.uint32)
        clipped, blanked, ms = _u64(0), _u64(0), C.c_float(0.0)
        _check(_agc(self._h, int(nsamp), int(sample_size), _vp(device_ptr), C.byref(cfg) if cfg is not None else None,
                    C.byref(state) if state is not None else None, int(out_sample_size), _vp(dst_device_ptr), _vp(stream or 0), _p(mults),
                    C.byref(clipped), C.byref(blanked), C.byref(ms)))
        return int(clipped.value), int(blanked.value), mults[:nwin], float(ms.value)

    def generate_batch_agc(self, desc, nsamp, fs, sample_size, cfg, out_sample_size, state=None, host_ptr=None, block_stride=None, carr_out=None):
        """gpsiq_generate_batch_agc: the run-ahead call rendered at sample_size and taken through gpsiq_agc on the device, with blocks of
        nsamp samples of out_sample_size in host memory; state as agc().  Returns (int8 / int16 [nblocks][2 * nsamp], elements the clamp
        changed, samples blanked), the array None when host_ptr names the caller's buffer (pageable or page-locked; block_stride bytes
        between blocks, default: back to back)."""
        desc = np.ascontiguousarray(desc, dtype=CHAN_DTYPE)
        nb, nc = desc.shape
        rlen = 2 * int(nsamp) * int(out_sample_size)
        stride = rlen if block_stride is None else int(block_stride)
        co = None if carr_out is None else _p(carr_out)
        clipped, blanked = _u64(0), _u64(0)
        out = None if host_ptr is not None else np.zeros((nb, max(stride, 1)), dtype=np.uint8)
        _check(_generate_batch_agc(self._h, _p(desc), nb, nc, int(nsamp), float(fs), int(sample_size), C.byref(cfg) if cfg is not None else None,
                                   C.byref(state) if state is not None else None, int(out_sample_size), _vp(host_ptr) if out is None else _p(out),
                                   stride, C.byref(clipped), C.byref(blanked), co))
        if out is None:
            return None, int(clipped.value), int(blanked.value)
        return (np.ascontiguousarray(out[:, :rlen]).view(np.int8 if int(out_sample_size) == 1 else np.int16), int(clipped.value),
                int(blanked.value))

    def agc_last_plan(self):
        """What the last agc() / generate_batch_agc() took: (grid of agc_measure or None, samples of a tile, grid of agc_gains, grid of
        agc_apply, samples of one of its workgroups, pieces)."""
        out = (C.c_longlong * 6)()
        _check(_agc_last_plan(self._h, out))
        return (None if out[0] < 0 else int(out[0])), int(out[1]), int(out[2]), int(out[3]), int(out[4]), int(out[5])

    def agc_last_ms(self):
        """Device milliseconds of the three launches of the last agc() that launched anything: (agc_measure, agc_gains, agc_apply)."""
        out = (C.c_float * 3)()
        _check(_agc_last_ms(self._h, out))
        return float(out[0]), float(out[1]), float(out[2])

    def pack_last_plan(self):
        """What the last pack() / unpack() / generate_batch_packed() took: (grid or None, units per block, tiles per block, pieces)."""
        out = (C.c_long * 4)()
        _check(_pack_last_plan(self._h, out))
        return (None if out[0] < 0 else int(out[0])), int(out[1]), int(out[2]), int(out[3])

    def synchronize(self, stream=None):
        _check(_synchronize(self._h, _vp(stream or 0)))

    def time_launches(self, block0, nblocks, nsamp, sample_size, device_ptr, block_stride, iters,
                      stream=None, variant=0):
        ms = C.c_float(0.0)
        _check(_time_launches(self._h, int(block0), int(nblocks), int(nsamp), int(sample_size), _vp(device_ptr),
                              int(block_stride), _vp(stream or 0), int(variant), int(iters),
                              C.byref(ms)))
        return ms.value
