"""
ctypes binding of libvgpa_hip.so (include/vgpa_hip.h).  Thin: argument marshalling, error mapping,
and a `Context` object that owns one `vgpa_ctx*`.

There is no CPU fallback here or anywhere in this package: if the shared library is missing, or no
HIP device is visible, the calls raise.
"""
import os
import ctypes
from ctypes import c_int, c_int32, c_int64, c_uint64, c_double, c_void_p, c_char_p, POINTER, byref

import numpy as np

ABI_VERSION = 2
# VGPA_LIB: another build of the same library (same-box A/B of build variants: tools/build_variant.sh); never set by the package
LIB_PATH = os.environ.get("VGPA_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libvgpa_hip.so")

MODEL_IDS = {"NONE": -1, "OU": 0, "DW": 1, "L63": 2, "L96": 3}
METHOD_IDS = {"euler": 0, "heun": 1, "rk2": 2, "rk4": 3}
PATH_KINDS = {"posterior": 0, "model": 1}
LAG_KINDS = {"covariance": 0, "propagator": 1}
FETCH_IDS = {"mt": 0, "st": 1, "lamt": 2, "psit": 3, "Efx": 4, "Edf": 5, "dEsde_dm": 6, "dEsde_ds": 7, "Esde_t": 8}
FLAG_FORCE_GENERIC = 1
FLAG_STREAM_LARGE_D = 4
FLAG_LIBRARY_GEMM = 8
FLAG_SYM_UNITS = 16
FLAG_KEEP_PSI = 32
FLAG_MATERIALIZE = 64
OPT_LD_CHUNK = 1
# vgpa_path_info: the values of its enum fields by name
STEPPER_IDS = {"large_d": 0, "lane": 1, "wave": 2, "mfma": 3, "generic": 4}
MOMENTS_IDS = {"row_major": 0, "time_major": 1}
LAYOUT_IDS = {"whole": 0, "upper": 1, "packed": 2}
BWD_IDS = {"none": 0, "psi": 1, "q": 2}

MAX_MARGINAL_LEVELS = 63      # kMaxMarginalLevels of the library: a bin is found with at most 6 compares

# exported symbols, checked by the CPU test-suite against include/vgpa_hip.h
SYMBOLS = ["vgpa_create", "vgpa_destroy", "vgpa_last_error", "vgpa_abi_version", "vgpa_device_count",
           "vgpa_synchronize", "vgpa_stream", "vgpa_solve_fwd", "vgpa_solve_bwd", "vgpa_energy",
           "vgpa_obs_energy", "vgpa_free_energy", "vgpa_gradient", "vgpa_sweep", "vgpa_energy_parts",
           "vgpa_fetch", "vgpa_theta_gradient", "vgpa_lag_covariance", "vgpa_sample_paths", "vgpa_sample_paths_weighted", "vgpa_particle_filter", "vgpa_particle_statistics", "vgpa_particle_events", "vgpa_particle_moments", "vgpa_particle_covariance", "vgpa_particle_marginals", "vgpa_particle_lag_covariance", "vgpa_path_cross_moments", "vgpa_particle_paths", "vgpa_particle_backward_paths", "vgpa_particle_backward_moments", "vgpa_particle_replaced_logw", "vgpa_particle_conditional", "vgpa_particle_forecast", "vgpa_sweep_dev", "vgpa_free_energy_dev", "vgpa_sweep_enqueue", "vgpa_fetch_f",
           "vgpa_dev_alloc", "vgpa_dev_free", "vgpa_memcpy_h2d", "vgpa_memcpy_d2h",
           "vgpa_profile_begin", "vgpa_profile_end", "vgpa_ld_gemm", "vgpa_ld_stage", "vgpa_gradient_dev", "vgpa_energy_full", "vgpa_set_option", "vgpa_is_streaming", "vgpa_path_info", "vgpa_set_prior_energy",
           "vgpa_set_problem_data", "vgpa_set_problem_params", "vgpa_set_problem_obs_model",
           "vgpa_vec_dot", "vgpa_vec_absmax", "vgpa_vec_asum", "vgpa_vec_axpby", "vgpa_release_x",
           "vgpa_shard_create", "vgpa_shard_destroy", "vgpa_shard_time_slice", "vgpa_shard_stream", "vgpa_shard_synchronize",
           "vgpa_shard_solve_fwd", "vgpa_shard_solve_bwd", "vgpa_shard_sweep", "vgpa_shard_sweep_sharded", "vgpa_shard_set_option",
           "vgpa_shard_get_option", "vgpa_shard_time_collectives", "vgpa_ld_gemm_chunk", "vgpa_rccl_unique_id", "vgpa_rccl_comm_create",
           "vgpa_rccl_comm_destroy", "vgpa_rccl_comm_count", "vgpa_rccl_comm_streams", "vgpa_shard_time_stage", "vgpa_shard_phase_ms", "vgpa_time_slice",
           "vgpa_device_alloc", "vgpa_device_free", "vgpa_device_memcpy", "vgpa_ld_launch_counts"]
# vgpa_ld_launch_counts: the counters in the order of the header's VGPA_LD_COUNT_* (the stage product: tile height x VGPA_LD_GEMM_*)
LD_GEMM_FORMS = ("checked", "full", "vec", "vec4", "seg", "seg4")
LD_COUNT_NAMES = (("stage_prod_fwd", "stage_prod_fwd_mid", "stage_prod_bwd", "stage_prod_bwd_mid", "stage_wide_fwd", "stage_wide_bwd",
                   "stage_sym", "stage_rows", "mid", "transpose", "library_gemm", "mid_cols") +
                  tuple(f"gemm{h}_{form}" for h in (32, 64, 128) for form in LD_GEMM_FORMS))

P_DOUBLE = POINTER(c_double)


class LdStageArgs(ctypes.Structure):
    """vgpa_ld_stage_args (include/vgpa_hip.h)."""
    _fields_ = [("D", c_int32), ("row0", c_int32), ("Mp", c_int32), ("cw", c_int32), ("fwd", c_int32),
                ("kstore", c_int32), ("final_mode", c_int32), ("lda", c_int32), ("cx", c_double), ("cf", c_double),
                ("W", c_void_p), ("Wcol", c_void_p), ("E0", c_void_p), ("E1", c_void_p), ("J", c_void_p),
                ("base", c_void_p), ("K1", c_void_p), ("K23", c_void_p), ("out", c_void_p), ("A0", c_void_p),
                ("A1", c_void_p), ("x", c_void_p), ("e0", c_void_p), ("e1", c_void_p), ("jv", c_void_p),
                ("vbase", c_void_p), ("k1v", c_void_p), ("k23v", c_void_p), ("vout", c_void_p)]


COMM_COLLECTIVE = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p)
COMM_GROUP = ctypes.CFUNCTYPE(c_int, c_void_p)
COMM_P2P = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_uint64, c_int, c_void_p)
SHARD_OPT_GATHER_CHUNKS, SHARD_OPT_TIMEOUT_MS = 1, 2


class VgpaComm(ctypes.Structure):
    """vgpa_comm (include/vgpa_hip.h): the collectives of the row-sharded recursion as a table of function pointers."""
    _fields_ = [("user", c_void_p), ("all_gather", COMM_COLLECTIVE), ("all_to_all", COMM_COLLECTIVE),
                ("group_begin", COMM_GROUP), ("group_end", COMM_GROUP), ("send", COMM_P2P), ("recv", COMM_P2P),
                ("abort", COMM_GROUP)]


class VgpaShardProblem(ctypes.Structure):
    """vgpa_shard_problem (include/vgpa_hip.h): what the fused row-sharded sweep needs besides x (device pointers, obs_t host)."""
    _fields_ = [("theta", c_double), ("inv_sigma_diag", c_void_p), ("m0", c_void_p), ("s0", c_void_p), ("sigma", c_void_p),
                ("n_obs", c_int32), ("obs_t", POINTER(c_int64)), ("obs_y", c_void_p), ("obs_rinv_diag", c_void_p),
                ("obs_const", c_double), ("e0", c_double)]


class VgpaPath(ctypes.Structure):
    """vgpa_path (include/vgpa_hip.h): the context's plan, then its record of what the buffers hold."""
    PLAN = ("fwd", "bwd", "sym_units", "launch_sym_units", "lane_pass", "bwd_upper", "store_q", "packed", "grad_in_bwd",
            "grad_in_bwd_now")
    RESIDENT = ("cached", "moments", "S", "dEs", "bwd_holds", "terms")
    PLAN_TAIL = ("helper_roles",)      # (the struct only ever grows at its end)
    _fields_ = [(name, c_int32) for name in PLAN + RESIDENT + PLAN_TAIL]


class VgpaConfig(ctypes.Structure):
    _fields_ = [("abi_version", c_int32), ("device", c_int32), ("model", c_int32), ("method", c_int32),
                ("dim_d", c_int32), ("n_pts", c_int32), ("batch", c_int32), ("flags", c_int32),
                ("dt", c_double), ("n_theta", c_int32), ("n_obs", c_int32),
                ("theta", P_DOUBLE), ("sigma", P_DOUBLE), ("m0", P_DOUBLE), ("s0", P_DOUBLE),
                ("obs_t", POINTER(c_int64)), ("obs_y", P_DOUBLE), ("obs_noise", P_DOUBLE), ("obs_h", P_DOUBLE),
                ("e0", c_double)]


_lib = None


def load():
    """Loads (once) and returns the ctypes handle of libvgpa_hip.so; fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m vgpa_amd.build` "
                           "(vgpa_amd has no CPU fallback).")
    # PyTorch bundles its own HIP runtime with the same SONAME (libamdhip64.so.7).  When torch is used in
    # this process (bench.py, torch.distributed) it must be imported first so that one runtime is shared.
    if os.environ.get("VGPA_PRELOAD_TORCH", "0") == "1":
        import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    lib.vgpa_last_error.restype = c_char_p
    lib.vgpa_last_error.argtypes = [c_void_p]
    lib.vgpa_stream.restype = c_void_p
    lib.vgpa_stream.argtypes = [c_void_p]
    lib.vgpa_create.argtypes = [POINTER(c_void_p), POINTER(VgpaConfig)]
    lib.vgpa_destroy.argtypes = [c_void_p]
    lib.vgpa_destroy.restype = None
    lib.vgpa_synchronize.argtypes = [c_void_p]
    lib.vgpa_solve_fwd.argtypes = [c_void_p] + [c_void_p] * 7
    lib.vgpa_solve_bwd.argtypes = [c_void_p] + [c_void_p] * 7
    lib.vgpa_energy.argtypes = [c_void_p] + [c_void_p] * 9
    lib.vgpa_obs_energy.argtypes = [c_void_p] + [c_void_p] * 5
    lib.vgpa_energy_full.argtypes = [c_void_p] + [c_void_p] * 11
    lib.vgpa_free_energy.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.vgpa_gradient.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.vgpa_sweep.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_energy_parts.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_fetch.argtypes = [c_void_p, c_int, c_void_p]
    lib.vgpa_theta_gradient.argtypes = [c_void_p, c_void_p]
    lib.vgpa_lag_covariance.argtypes = [c_void_p, c_int, c_void_p, c_int32, POINTER(c_int64), c_int32, c_void_p]
    lib.vgpa_sample_paths.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_void_p]
    lib.vgpa_sample_paths_weighted.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_filter.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_statistics.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_events.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_moments.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_covariance.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_marginals.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_int32,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_lag_covariance.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_int32, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_path_cross_moments.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_paths.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_uint64, c_double, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_backward_paths.argtypes = lib.vgpa_particle_paths.argtypes
    lib.vgpa_particle_backward_moments.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_replaced_logw.argtypes = [c_void_p, c_int32, c_void_p]
    lib.vgpa_particle_conditional.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_particle_forecast.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_uint64, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                           c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p]
    lib.vgpa_sweep_dev.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_free_energy_dev.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.vgpa_sweep_enqueue.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.vgpa_fetch_f.argtypes = [c_void_p, c_void_p]
    lib.vgpa_dev_alloc.argtypes = [c_void_p, c_uint64, POINTER(c_void_p)]
    lib.vgpa_dev_free.argtypes = [c_void_p, c_void_p]
    lib.vgpa_memcpy_h2d.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64]
    lib.vgpa_memcpy_d2h.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64]
    lib.vgpa_ld_gemm.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                 c_void_p, c_int]
    lib.vgpa_ld_stage.argtypes = [c_void_p, POINTER(LdStageArgs)]
    lib.vgpa_gradient_dev.argtypes = [c_void_p, c_void_p]
    lib.vgpa_release_x.argtypes = [c_void_p]
    lib.vgpa_shard_create.argtypes = [POINTER(c_void_p), c_int, c_double, c_int, c_int, c_int, c_int, c_int,
                                      POINTER(VgpaComm), c_void_p]
    lib.vgpa_shard_destroy.argtypes = [c_void_p]
    lib.vgpa_shard_destroy.restype = None
    lib.vgpa_shard_time_slice.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.vgpa_shard_stream.argtypes = [c_void_p]
    lib.vgpa_shard_stream.restype = c_void_p
    lib.vgpa_shard_synchronize.argtypes = [c_void_p]
    lib.vgpa_shard_solve_fwd.argtypes = [c_void_p] + [c_void_p] * 7
    lib.vgpa_shard_solve_bwd.argtypes = [c_void_p] + [c_void_p] * 7
    lib.vgpa_shard_sweep.argtypes = [c_void_p, POINTER(VgpaShardProblem), c_void_p, P_DOUBLE, c_void_p, c_void_p]
    lib.vgpa_shard_sweep.restype = c_int
    lib.vgpa_shard_sweep_sharded.argtypes = [c_void_p, POINTER(VgpaShardProblem), c_void_p, c_void_p, P_DOUBLE, c_void_p, c_void_p]
    lib.vgpa_shard_set_option.argtypes = [c_void_p, c_int, c_int64]
    lib.vgpa_shard_get_option.argtypes = [c_void_p, c_int, POINTER(c_int64)]
    lib.vgpa_shard_time_collectives.argtypes = [c_void_p, c_int, P_DOUBLE, P_DOUBLE]
    lib.vgpa_ld_gemm_chunk.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                       c_int, c_int, c_int]
    lib.vgpa_ld_launch_counts.argtypes = [POINTER(c_int64), c_int]
    lib.vgpa_rccl_unique_id.argtypes = [c_void_p]
    lib.vgpa_rccl_comm_create.argtypes = [POINTER(VgpaComm), c_void_p, c_int, c_int, c_int]
    lib.vgpa_rccl_comm_destroy.argtypes = [POINTER(VgpaComm)]
    lib.vgpa_rccl_comm_destroy.restype = None
    lib.vgpa_rccl_comm_count.argtypes = [POINTER(VgpaComm), POINTER(c_int)]
    lib.vgpa_rccl_comm_streams.argtypes = [POINTER(VgpaComm), POINTER(c_int)]
    lib.vgpa_shard_time_stage.argtypes = [c_void_p, c_int, c_int, P_DOUBLE]
    lib.vgpa_shard_phase_ms.argtypes = [c_void_p, P_DOUBLE]
    lib.vgpa_time_slice.argtypes = [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]
    lib.vgpa_device_alloc.argtypes = [c_int, c_uint64, POINTER(c_void_p)]
    lib.vgpa_device_free.argtypes = [c_int, c_void_p]
    lib.vgpa_device_memcpy.argtypes = [c_int, c_void_p, c_void_p, c_uint64, c_int]
    lib.vgpa_vec_dot.argtypes = [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]
    lib.vgpa_vec_absmax.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p]
    lib.vgpa_vec_asum.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p]
    lib.vgpa_vec_axpby.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vgpa_set_option.argtypes = [c_void_p, c_int, c_int64]
    lib.vgpa_is_streaming.argtypes = [c_void_p]
    lib.vgpa_path_info.argtypes = [c_void_p, POINTER(VgpaPath)]
    lib.vgpa_set_prior_energy.argtypes = [c_void_p, c_double]
    lib.vgpa_set_problem_data.argtypes = [c_void_p] + [c_void_p] * 5
    lib.vgpa_set_problem_params.argtypes = [c_void_p] + [c_void_p] * 2
    lib.vgpa_set_problem_obs_model.argtypes = [c_void_p] + [c_void_p] * 3
    lib.vgpa_profile_begin.argtypes = [c_void_p]
    lib.vgpa_profile_end.argtypes = [c_void_p, P_DOUBLE, P_DOUBLE, P_DOUBLE, P_DOUBLE, POINTER(c_int64)]
    abi = lib.vgpa_abi_version()
    if abi != ABI_VERSION:
        raise RuntimeError(f"libvgpa_hip ABI {abi} != binding ABI {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def device_count():
    return int(load().vgpa_device_count())


def _raise(code, msg):
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    if code == -1:
        raise ValueError(msg)
    if code == -3:
        raise np.linalg.LinAlgError(msg)
    if code == -5:
        raise NotImplementedError(msg)
    if code == -6:
        raise RuntimeError(f"libvgpa_hip: a collective of the row-sharded path failed or timed out; the communicator was aborted "
                           f"and this shard is unusable ({msg})")
    raise RuntimeError(f"libvgpa_hip error {code}: {msg}")


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _arg(a):
    """an input of an entry point as ctypes takes it: an integer as it is, an array (or None) as its pointer"""
    return a if type(a) is int else _ptr(a)


def _shaped(a, shape, name, dtype=np.float64):
    """A per-problem input as a contiguous array of exactly `shape`, or None; int64 inputs must hold integer grid indices."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.shape != shape:
        raise ValueError(f"{name} has shape {a.shape}, expected {shape}")
    if dtype == np.int64 and a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must hold integer grid indices")
    return np.ascontiguousarray(a, dtype=dtype)


def per_problem(a, batch, d):
    """Levels or sides of the path events, one row per problem: (batch, d), or (d,) or a scalar for every problem, as a (batch, d) view"""
    a = np.asarray(a)
    return np.broadcast_to(a.reshape(-1, d) if a.size > 1 else a.reshape(1, 1), (batch, d))


class DeviceBuffer:
    """A caller-owned device allocation (fp64) on the context's device."""

    def __init__(self, ctx, count):
        self.ctx, self.count = ctx, int(count)
        p = c_void_p()
        ctx._check(ctx._lib.vgpa_dev_alloc(ctx._h, self.count * 8, byref(p)))
        self.ptr = p

    def upload(self, host):
        host = _c64(host).ravel()
        assert host.size == self.count
        self.ctx._check(self.ctx._lib.vgpa_memcpy_h2d(self.ctx._h, self.ptr, _ptr(host), host.size * 8))

    def upload_at(self, offset, host):
        """host -> this buffer from double `offset` on (large batches go up in pieces instead of through one host array)."""
        host = _c64(host).ravel()
        assert 0 <= offset and offset + host.size <= self.count
        dst = c_void_p(self.ptr.value + 8 * int(offset))
        self.ctx._check(self.ctx._lib.vgpa_memcpy_h2d(self.ctx._h, dst, _ptr(host), host.size * 8))

    def download_at(self, offset, count):
        out = np.empty(int(count))
        assert 0 <= offset and offset + out.size <= self.count
        src = c_void_p(self.ptr.value + 8 * int(offset))
        self.ctx._check(self.ctx._lib.vgpa_memcpy_d2h(self.ctx._h, _ptr(out), src, out.size * 8))
        return out

    def download(self):
        out = np.empty(self.count)
        self.ctx._check(self.ctx._lib.vgpa_memcpy_d2h(self.ctx._h, _ptr(out), self.ptr, out.size * 8))
        return out

    def free(self):
        if self.ptr and self.ctx._h is not None:
            self.ctx._lib.vgpa_dev_free(self.ctx._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostArray:
    """What `DeviceArray.cpu()` returns: the data on the host (`.numpy()`), so that callers written against a tensor
    library's `.cpu().numpy()` read the same."""

    def __init__(self, a):
        self._a = a

    def numpy(self):
        return self._a


class DeviceArray:
    """An fp64 array in device memory owned by this object (vgpa_device_alloc; freed with it), with just enough surface for the
    callers of the row-sharded driver: `.ptr` / `.data_ptr()`, `.shape`, `[:n]` views of the leading dimension, `.numpy()` /
    `.cpu().numpy()` (download), and `__cuda_array_interface__`, through which a tensor library can wrap the memory without a copy
    (`torch.as_tensor(arr, device="cuda")`)."""

    def __init__(self, shape, device=0, _base=None, _ptr=None):
        self.shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.device = int(device)
        self._lib = load()
        self._base = _base                       # a view keeps its owner alive
        if _base is None:
            p = c_void_p()
            rc = self._lib.vgpa_device_alloc(self.device, max(self.size, 1) * 8, byref(p))
            if rc != 0:
                _raise(rc, f"vgpa_device_alloc({self.size * 8} bytes) failed")
            self.ptr = p.value
        else:
            self.ptr = int(_ptr)

    @property
    def size(self):
        n = 1
        for v in self.shape:
            n *= v
        return n

    @classmethod
    def from_host(cls, a, device=0):
        a = _c64(a)
        out = cls(a.shape, device)
        rc = out._lib.vgpa_device_memcpy(out.device, c_void_p(out.ptr), _ptr(a), a.size * 8, 1)
        if rc != 0:
            _raise(rc, "vgpa_device_memcpy (host -> device) failed")
        return out

    def data_ptr(self):
        return self.ptr

    def numpy(self):
        out = np.empty(self.shape)
        rc = self._lib.vgpa_device_memcpy(self.device, _ptr(out), c_void_p(self.ptr), out.size * 8, 2)
        if rc != 0:
            _raise(rc, "vgpa_device_memcpy (device -> host) failed")
        return out

    def cpu(self):
        return HostArray(self.numpy())

    def __getitem__(self, key):
        if not (isinstance(key, slice) and key.step in (None, 1)):
            raise TypeError("DeviceArray supports contiguous slices of the leading dimension only")
        lo, hi, _ = key.indices(self.shape[0])
        hi = max(hi, lo)
        inner = self.size // self.shape[0] if self.shape[0] else 0
        return DeviceArray((hi - lo,) + self.shape[1:], self.device, _base=self if self._base is None else self._base,
                           _ptr=self.ptr + 8 * lo * inner)

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": "<f8", "data": (self.ptr, False), "version": 3, "strides": None}

    def __del__(self):
        try:
            if self._base is None and getattr(self, "ptr", None):
                self._lib.vgpa_device_free(self.device, c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


class ExternalBuffer:
    """A device allocation owned by someone else (e.g. a torch tensor's storage), passed by raw pointer."""

    def __init__(self, ptr, count):
        self.ptr, self.count = c_void_p(int(ptr)), int(count)


class Context:
    """
    Owns one vgpa_ctx.  `model` in {"NONE","OU","DW","L63","L96"}, `method` in {"euler","heun","rk2","rk4"}.
    Leave m0/s0/obs_* as None for an ODE-only context (solve_fwd / solve_bwd / energy operators).
    """

    def __init__(self, model, method, dim_d, n_pts, dt, sigma, theta=None, m0=None, s0=None, obs_t=None,
                 obs_y=None, obs_noise=None, obs_h=None, e0=0.0, batch=1, device=0, flags=0):
        self._lib = load()
        self._h = None
        self.model, self.method = str(model).upper(), str(method).lower()
        if self.model not in MODEL_IDS:
            raise ValueError(f" Unknown stochastic model -> {model}")
        if self.method not in METHOD_IDS:
            raise ValueError(f" Integration method is unknown -> {method}.")
        self.D, self.Np, self.B = int(dim_d), int(n_pts), int(batch)
        self.len_x = self.Np * self.D * (self.D + 1)
        keep = []

        def arr(a, n=None, dtype=np.float64):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=dtype)).ravel()
            if n is not None and a.size != n:
                raise ValueError(f"bad array size {a.size}, expected {n}")
            keep.append(a)
            return a

        d, dd = self.D, self.D * self.D
        theta_a = arr(np.atleast_1d(theta)) if theta is not None else None
        obs_t_a = arr(obs_t, dtype=np.int64)
        n_obs = 0 if obs_t_a is None else obs_t_a.size
        cfg = VgpaConfig()
        cfg.abi_version, cfg.device = ABI_VERSION, int(device)
        cfg.model, cfg.method = MODEL_IDS[self.model], METHOD_IDS[self.method]
        cfg.dim_d, cfg.n_pts, cfg.batch, cfg.flags = d, self.Np, self.B, int(flags)
        cfg.dt = float(dt)
        cfg.n_theta = 0 if theta_a is None else theta_a.size
        cfg.n_obs = n_obs
        cfg.e0 = float(e0)

        def dp(a):
            return None if a is None else a.ctypes.data_as(P_DOUBLE)

        cfg.theta = dp(theta_a)
        cfg.sigma = dp(arr(sigma, dd))
        cfg.m0 = dp(arr(m0, d))
        cfg.s0 = dp(arr(s0, dd))
        cfg.obs_t = None if obs_t_a is None else obs_t_a.ctypes.data_as(POINTER(c_int64))
        cfg.obs_y = dp(arr(obs_y, n_obs * d if obs_y is not None else None))
        cfg.obs_noise = dp(arr(obs_noise, dd))
        cfg.obs_h = dp(arr(obs_h, dd))
        h = c_void_p()
        rc = self._lib.vgpa_create(byref(h), byref(cfg))
        if rc != 0:
            _raise(rc, self._lib.vgpa_last_error(None))
        self._h = h
        self.n_obs = n_obs
        self.n_theta = cfg.n_theta

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            _raise(rc, self._lib.vgpa_last_error(self._h))

    def close(self):
        if self._h is not None:
            self._lib.vgpa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape_v(self):
        return (self.B, self.Np, self.D)

    def _shape_m(self):
        return (self.B, self.Np, self.D, self.D)

    def _squeeze(self, a):
        return a[0] if self.B == 1 else a

    # ------------------------------------------------------------------ operator level
    def solve_fwd(self, lin_a, off_b, m0, s0, sigma):
        a, b = _c64(lin_a), _c64(off_b)
        m0, s0, sigma = _c64(m0), _c64(s0), _c64(sigma)
        mt, st = np.empty(self._shape_v()), np.empty(self._shape_m())
        self._check(self._lib.vgpa_solve_fwd(self._h, _ptr(a), _ptr(b), _ptr(m0), _ptr(s0), _ptr(sigma),
                                             _ptr(mt), _ptr(st)))
        return self._squeeze(mt), self._squeeze(st)

    def solve_bwd(self, lin_a, de_dm, de_ds, jm, js):
        a, em, es, jm, js = (_c64(v) for v in (lin_a, de_dm, de_ds, jm, js))
        lam, psi = np.empty(self._shape_v()), np.empty(self._shape_m())
        self._check(self._lib.vgpa_solve_bwd(self._h, _ptr(a), _ptr(em), _ptr(es), _ptr(jm), _ptr(js),
                                             _ptr(lam), _ptr(psi)))
        return self._squeeze(lam), self._squeeze(psi)

    def energy(self, lin_a, off_b, mt, st, want_edf=True, want_hyper=False):
        """(Esde, Ef, Edf, dEsde_dm, dEsde_ds[, dEsde_dth, dEsde_dSig]) -- the last two with want_hyper."""
        a, b, m, s = (_c64(v) for v in (lin_a, off_b, mt, st))
        esde = np.empty(self.B)
        ef, dm = np.empty(self._shape_v()), np.empty(self._shape_v())
        edf = np.empty(self._shape_m()) if want_edf else None
        ds = np.empty(self._shape_m())
        dth = dsg = None
        if want_hyper:
            dth = np.empty(self.B) if self.D == 1 else np.empty((self.B, self.D))
            dsg = np.empty(self.B) if self.D == 1 else np.empty((self.B, self.D, self.D))
        self._check(self._lib.vgpa_energy_full(self._h, _ptr(a), _ptr(b), _ptr(m), _ptr(s), _ptr(esde), _ptr(ef),
                                               _ptr(edf), _ptr(dm), _ptr(ds), _ptr(dth), _ptr(dsg)))
        sq = self._squeeze
        out = ((float(esde[0]) if self.B == 1 else esde), sq(ef), (sq(edf) if want_edf else None), sq(dm), sq(ds))
        if want_hyper:
            one = self.B == 1
            out += ((float(dth[0]) if self.D == 1 else dth[0]) if one else dth,
                    (float(dsg[0]) if self.D == 1 else dsg[0]) if one else dsg)
        return out

    def obs_energy(self, mt, st, want_jumps=True):
        m, s = _c64(mt), _c64(st)
        eobs = np.empty(self.B)
        jm = np.empty(self._shape_v()) if want_jumps else None
        js = np.empty(self._shape_m()) if want_jumps else None
        self._check(self._lib.vgpa_obs_energy(self._h, _ptr(m), _ptr(s), _ptr(eobs), _ptr(jm), _ptr(js)))
        e = float(eobs[0]) if self.B == 1 else eobs
        if not want_jumps:
            return e
        return e, self._squeeze(jm), self._squeeze(js)

    # ------------------------------------------------------------------ fused objective
    def free_energy(self, x):
        x = _c64(x)
        if x.size != self.B * self.len_x:
            raise ValueError(f"x has {x.size} entries, expected {self.B * self.len_x}")
        f = np.empty(self.B)
        self._check(self._lib.vgpa_free_energy(self._h, _ptr(x), _ptr(f)))
        return float(f[0]) if self.B == 1 else f

    def gradient(self, x=None):
        g = np.empty(self.B * self.len_x)
        xx = None if x is None else _c64(x)
        self._check(self._lib.vgpa_gradient(self._h, _ptr(xx), _ptr(g)))
        return g if self.B == 1 else g.reshape(self.B, self.len_x)

    def sweep(self, x):
        x = _c64(x)
        if x.size != self.B * self.len_x:
            raise ValueError(f"x has {x.size} entries, expected {self.B * self.len_x}")
        f, g = np.empty(self.B), np.empty(self.B * self.len_x)
        self._check(self._lib.vgpa_sweep(self._h, _ptr(x), _ptr(f), _ptr(g)))
        if self.B == 1:
            return float(f[0]), g
        return f, g.reshape(self.B, self.len_x)

    def energy_parts(self):
        """(e0, E_sde, E_obs) of the cached state, each (B,) (floats at B = 1); e0 is every problem's own."""
        e0, es, eo = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        self._check(self._lib.vgpa_energy_parts(self._h, _ptr(e0), _ptr(es), _ptr(eo)))
        if self.B == 1:
            return float(e0[0]), float(es[0]), float(eo[0])
        return e0, es, eo

    def theta_gradient(self):
        """dF/dtheta at fixed (A_t, b_t) from the state the last fused evaluation left resident: (n_theta,) at B = 1, else
        (B, n_theta).  The cached state survives (gradient(None), fetch, energy_parts afterwards are unchanged).  RuntimeError
        without a cached state, NotImplementedError in the time-chunked large-D sweep."""
        out = np.empty((self.B, max(self.n_theta, 1)))
        self._check(self._lib.vgpa_theta_gradient(self._h, _ptr(out)))
        return out[0] if self.B == 1 else out

    def _walk_inputs(self, x, x0, prior=None):
        """x, x0 and prior of a sampler call laid out for the C ABI: xx (B len_x), s0 (B, D), mu (B, D), tau (B, D, D), None where the argument is"""
        xx = None if x is None else _c64(x)
        if xx is not None and xx.size != self.B * self.len_x:
            raise ValueError(f"x has {xx.size} entries, expected {self.B * self.len_x}")
        s0 = None if x0 is None else _c64(np.broadcast_to(np.asarray(x0, dtype=np.float64).reshape(-1, self.D), (self.B, self.D)))
        mu = tau = None
        if prior is not None:
            mu = _c64(np.broadcast_to(np.asarray(prior[0], dtype=np.float64).reshape(-1, self.D), (self.B, self.D)))
            tau = _c64(np.broadcast_to(np.asarray(prior[1], dtype=np.float64).reshape(-1, self.D, self.D), (self.B, self.D, self.D)))
        return xx, s0, mu, tau

    def _filter_outputs(self, n):
        """the filter's results for n particles, to be filled by the library: log_w (B, n), state (B, n, D), ess (B, M), resampled (B, M) int32"""
        m = self.n_obs
        return np.empty((self.B, n)), np.empty((self.B, n, self.D)), np.zeros((self.B, m)), np.zeros((self.B, m), dtype=np.int32)

    @staticmethod
    def _fit32(**named):
        """the C ABI takes int32: nothing may wrap on its way there (ctypes wraps silently)"""
        if not all(-2 ** 31 <= v < 2 ** 31 for v in named.values()):
            names = list(named)
            raise ValueError(f"{' and '.join(filter(None, (', '.join(names[:-1]), names[-1])))} must fit into 32 bits ("
                             + ", ".join(f"{k} = {v}" for k, v in named.items()) + ")")

    def _slot_array(self, slots, k):
        """slots (B, k) or (k,) as the (B, k) int32 array of the C ABI; None stays None"""
        if slots is None:
            return None
        wide = np.asarray(slots)
        if wide.dtype.kind not in "iu" or wide.size == 0 or wide.min() < -2 ** 31 or wide.max() >= 2 ** 31:
            raise ValueError("slots must be integers that fit into 32 bits")
        return np.ascontiguousarray(np.broadcast_to(wide.reshape(-1, k), (self.B, k)), dtype=np.int32)

    def _n_keep(self, stride):
        """the number of kept grid indices 0, stride, 2 stride, ... (the library refuses a stride below 1)"""
        return (self.Np - 1) // max(stride, 1) + 1

    @staticmethod
    def _seed(seed):
        return int(seed) & 0xFFFFFFFFFFFFFFFF

    def _new(self, *shape, fill=None, dtype=np.float64):
        """a result (B, *shape) for the library to write: as it comes, or holding `fill` where the library leaves entries as they are"""
        return np.empty((self.B,) + shape, dtype=dtype) if fill is None else np.full((self.B,) + shape, fill, dtype=dtype)

    def _history(self, n, wanted):
        """the filter's histories: ancestors (B, M, n) int32 of -1 and clouds (B, M, n, D) of NaN, or None and None"""
        return {"ancestors": self._new(self.n_obs, n, fill=-1, dtype=np.int32) if wanted else None,
                "clouds": self._new(self.n_obs, n, self.D, fill=np.nan) if wanted else None}

    def _filter_call(self, entry, ints, seed, ess_fraction, x, x0, prior, outputs=None, inputs=None, head=None, slots=None, history=None):
        """One call of the filter family.  All its entry points but the forecast have the shape
            (h, x, x0, [ref], n_paths, [n_draw, final_slots], [stride], seed, ess_fraction, mu, tau, [own inputs], logw, state, [own outputs],
             ess, resampled, [ancestors, clouds])
        and a method says what is its own: ints, the entry's integers by name (n_paths and, where it has them, n_draw and stride; with n_draw
        go the final `slots`); inputs() -> its own input arrays (and an integer that goes with them), checked before x; head() -> what stands before n_paths, checked behind x;
        outputs(n, k, n_keep) -> {key: array or None} in the entry's order; history: None where the entry has no histories, else whether they
        are wanted.  Returns the dict: log_w, state, ess, resampled, the histories, the entry's own."""
        ints = {name: int(v) for name, v in ints.items()}
        self._fit32(**ints)
        own_in = inputs() if inputs else ()
        xx, s0, mu, tau = self._walk_inputs(x, x0, prior)
        first = head() if head else ()
        n, k = max(ints["n_paths"], 0), max(ints.get("n_draw", 0), 0)
        draw = (ints["n_draw"], _ptr(self._slot_array(slots, k))) if "n_draw" in ints else ()
        log_w, state, ess, flags = self._filter_outputs(n)
        own = outputs(n, k, self._n_keep(ints.get("stride", 1))) if outputs else {}
        hist = {} if history is None else self._history(n, history)
        self._check(getattr(self._lib, entry)(self._h, _ptr(xx), _ptr(s0), *map(_ptr, first), ints["n_paths"], *draw,
                                              *((ints["stride"],) if "stride" in ints else ()), self._seed(seed), float(ess_fraction), _ptr(mu),
                                              _ptr(tau), *map(_arg, own_in), _ptr(log_w), _ptr(state), *map(_ptr, own.values()), _ptr(ess),
                                              _ptr(flags), *map(_ptr, hist.values())))
        return {"log_w": log_w, "state": state, "ess": ess, "resampled": flags, **hist, **own}

    def lag_covariance(self, anchors, kind="covariance", stride=1, x=None):
        """The two-time covariance K(k, s) = Phi(k, s) S_s of the posterior process (kind "covariance") or the propagator Phi(k, s) of
        dPhi/dt = -A_t Phi itself (kind "propagator") from every anchor s to the end of the grid (vgpa_lag_covariance): the context's scheme
        for the mean equation with b = 0, applied to every column.  anchors: strictly increasing grid indices.  x=None: the x of the cached
        evaluation, which stays as it is; the covariance kind with an x evaluates free_energy(x) first (its S_t is what the call reads), the
        propagator kind uploads x and drops the cached state.  Returns a LagCovariance: values (B, n_anchor, n_keep, D, D) at the grid
        indices 0, stride, ..., zero before each anchor."""
        from .lagcov import LagCovariance
        if kind not in LAG_KINDS:
            raise ValueError(f" Unknown kind of lag covariance -> {kind}")
        stride = int(stride)
        anc = np.asarray(anchors)
        if anc.ndim == 0:
            anc = anc.reshape(1)
        if anc.ndim != 1 or (anc.size and anc.dtype.kind not in "iu"):
            raise ValueError("anchors must be a 1-D sequence of integer grid indices")
        anc = np.ascontiguousarray(anc, dtype=np.int64)
        self._fit32(n_anchor=int(anc.size), stride=stride)
        xx = self._walk_inputs(x, None)[0]
        if xx is not None and kind == "covariance":
            self.free_energy(xx)
            xx = None
        n_keep = self._n_keep(stride)
        out = self._new(anc.size, n_keep, self.D, self.D)
        self._check(self._lib.vgpa_lag_covariance(self._h, LAG_KINDS[kind], _ptr(xx), int(anc.size),
                                                  anc.ctypes.data_as(POINTER(c_int64)) if anc.size else None, stride, _ptr(out)))
        return LagCovariance(out, anc, np.arange(n_keep) * stride, kind)

    def sample_paths(self, kind, n_paths, seed, stride=1, x=None, x0=None):
        """Euler-Maruyama paths on the context's grid: kind "posterior" (dx = (-A_t x + b_t) dt + Sigma^1/2 dW, from x or, x=None, the x of
        the cached evaluation, which stays as it is) or "model" (the model SDE at the theta in force; takes no x).  x0 (B, D): the start of every
        path of a problem; None: x_0 ~ N(m0, S0).  Returns (B, n_paths, n_keep, D), the grid points 0, stride, 2 stride, ...  The draws
        depend on (seed, problem, path, grid index, component) alone."""
        if kind not in PATH_KINDS:
            raise ValueError(f" Unknown kind of paths -> {kind}")
        n_paths, stride = int(n_paths), int(stride)
        self._fit32(n_paths=n_paths, stride=stride)
        xx, s0, _, _ = self._walk_inputs(x, x0)
        out = self._new(max(n_paths, 0), self._n_keep(stride), self.D)
        self._check(self._lib.vgpa_sample_paths(self._h, PATH_KINDS[kind], _ptr(xx), _ptr(s0), n_paths, stride, self._seed(seed), _ptr(out)))
        return out

    def sample_paths_weighted(self, n_paths, seed, stride=1, x=None, x0=None, paths=True):
        """The posterior paths of sample_paths with the same arguments and, per path, the two sums of its importance weight against the
        model SDE and the data (vgpa_sample_paths_weighted): (paths (B, n_paths, n_keep, D) or None, logw (B, n_paths, 2): the path term and
        the observation term, start (B, n_paths, D): every x_0).  paths=False: no path is stored or copied."""
        n_paths, stride = int(n_paths), int(stride)
        self._fit32(n_paths=n_paths, stride=stride)
        xx, s0, _, _ = self._walk_inputs(x, x0)
        n = max(n_paths, 0)
        out = self._new(n, self._n_keep(stride), self.D) if paths else None
        logw, start = self._new(n, 2), self._new(n, self.D)
        self._check(self._lib.vgpa_sample_paths_weighted(self._h, _ptr(xx), _ptr(s0), n_paths, stride, self._seed(seed), _ptr(out), _ptr(start),
                                                         _ptr(logw)))
        return out, logw, start

    def particle_filter(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, prior=None, history=False):
        """The guided particle filter (vgpa_particle_filter): the walk of sample_paths_weighted with the weights taken in observation by
        observation and the cloud resampled (systematic) whenever ESS < ess_fraction n_paths.  prior: (mu0 (B, D), tau0 (B, D, D)) for the
        initial term of a drawn start, or None.  Returns a dict: log_w (B, n_paths), state (B, n_paths, D), ess (B, M), resampled (B, M) int32
        and, history=True, ancestors (B, M, n_paths) int32 and clouds (B, M, n_paths, D) (else None), M = the context's n_obs.  Rows at or
        beyond a problem's own observation count: ess 0, resampled 0, ancestors -1, clouds NaN."""
        return self._filter_call("vgpa_particle_filter", {"n_paths": n_paths}, seed, ess_fraction, x, x0, prior, history=bool(history))

    def particle_statistics(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, prior=None, per_particle=False):
        """The path statistics of particle_filter's lineages (vgpa_particle_statistics): the same walk and resampling decisions, every slot
        carrying its row (Q, G, H) of sum_k r^2 / dt, sum_k phi r, sum_k dt phi^2.  Returns a dict: log_w, state, ess, resampled as
        particle_filter (bit for bit), mean (B, 3, D): the self-normalised weighted mean of the rows, reduced on the device, and stats
        (B, n_paths, 3, D): the rows themselves (per_particle=True, else None)."""
        return self._filter_call("vgpa_particle_statistics", {"n_paths": n_paths}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "stats": self._new(n, 3, self.D) if per_particle else None, "mean": self._new(3, self.D)})

    def _event_inputs(self, levels, side):
        """levels and side of particle_events laid out for the C ABI: (B, D) float64 and (B, D) int32.  A scalar or (D,) is every problem's."""
        lev = np.asarray(levels, dtype=np.float64)
        if lev.size not in (1, self.D, self.B * self.D):
            raise ValueError(f"levels has {lev.size} entries, expected 1, {self.D} or {self.B * self.D}")
        lev = _c64(per_problem(lev, self.B, self.D))
        if not np.all(np.isfinite(lev)):
            raise ValueError("levels must be finite")
        sd = np.asarray(side)
        if sd.size not in (1, self.D, self.B * self.D):
            raise ValueError(f"side has {sd.size} entries, expected 1, {self.D} or {self.B * self.D}")
        if not np.all((sd == 1) | (sd == -1)):
            raise ValueError("side must be +1 or -1")
        return lev, np.ascontiguousarray(per_problem(sd, self.B, self.D), dtype=np.int32)

    def particle_events(self, n_paths, seed, levels, side=1, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None, per_particle=False):
        """Path events of particle_filter's lineages (vgpa_particle_events): the same walk and resampling decisions, every slot carrying the
        row (X, T, N) of g_j(x) = side_j (x_j - levels_j) along its lineage: the largest g, the first grid index with g > 0 (Np: never) and
        the number of grid indices with g > 0.  levels, side: (B, D), or (D,) or a scalar for every problem; side is +1 (above the level) or
        -1 (below it).  Returns a dict: log_w, state, ess, resampled as particle_filter (bit for bit), mean (B, 3, D): the self-normalised
        weighted mean of the rows, cdf (B, n_keep, D): the weighted share of lineages with T <= k at the grid indices k = 0, stride, ...,
        both reduced on the device, and rows (B, n_paths, 3, D): the rows themselves (per_particle=True, else None)."""
        return self._filter_call("vgpa_particle_events", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "rows": self._new(n, 3, self.D) if per_particle else None, "mean": self._new(3, self.D), "cdf": self._new(n_keep, self.D)},
            inputs=lambda: self._event_inputs(levels, side))

    def particle_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None):
        """The smoothing moments on the grid under particle_filter's genealogy (vgpa_particle_moments): the filter, its final weights pushed
        back through the ancestors, and the walk once more with the weighted sums taken on the device.  Returns a dict: log_w, state, ess,
        resampled as particle_filter (bit for bit), moments (B, n_keep, 2, D): sum W x and sum W x^2 at the grid indices 0, stride, ...,
        and lineage_ess (B, M + 1): 1 / sum W^2 of every stretch between two observations (0 beyond a problem's own count + 1)."""
        return self._filter_call("vgpa_particle_moments", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "moments": self._new(n_keep, 2, self.D), "lineage_ess": self._new(self.n_obs + 1, fill=0.0)})

    def particle_backward_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None, weights=True):
        """The smoothing moments on the grid under the marginal backward smoother (vgpa_particle_backward_moments): particle_moments with the
        weights of every stretch taken from all n particles of particle_filter's stored clouds -- at every observation where the cloud was
        resampled W^j = W^{j+1} P, P the row-normalised table of filter weight times model transition density, the expectation of
        particle_backward_paths' draw -- and not from the lineages the resamplings have left.  Returns a dict: log_w, state, ess, resampled as
        particle_filter (bit for bit), moments (B, n_keep, 2, D) as particle_moments, smoothing_ess (B, M + 1): 1 / sum W^2 of every stretch
        (0 beyond a problem's own count + 1), and weights (B, M + 1, n_paths): the table itself (weights=True, else None).  Where nothing
        was resampled (ess_fraction=0, n_paths=1) moments are particle_moments' bit for bit; where the particles of a cloud lie many
        transition widths apart P is one-hot and the result is the genealogy's."""
        return self._filter_call("vgpa_particle_backward_moments", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "moments": self._new(n_keep, 2, self.D), "smoothing_ess": self._new(self.n_obs + 1, fill=0.0),
            "weights": self._new(self.n_obs + 1, n, fill=0.0) if weights else None})

    def particle_replaced_logw(self, n_paths):
        """(B, M, n_paths): the log-weights the resamplings of the last particle_backward_paths / particle_backward_moments call with this
        n_paths replaced (vgpa_particle_replaced_logw), the observation's term included; NaN where the cloud was carried on.  With
        particle_filter(history=True)'s ancestors and clouds: the histories the backward kernels read."""
        n_paths = int(n_paths)
        self._fit32(n_paths=n_paths)
        out = self._new(self.n_obs, max(n_paths, 0), fill=np.nan)
        self._check(self._lib.vgpa_particle_replaced_logw(self._h, n_paths, _ptr(out)))
        return out

    def particle_covariance(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None):
        """The smoothing mean and the full second-moment matrices on the grid under particle_filter's genealogy (vgpa_particle_covariance):
        particle_moments with every cross moment.  Returns a dict: log_w, state, ess, resampled as particle_filter (bit for bit), lineage_ess
        as particle_moments (bit for bit), mean (B, n_keep, D): sum W x, and second (B, n_keep, D, D): sum W x x^T, symmetric to the bit,
        at the grid indices 0, stride, ...  The covariance is second - mean mean^T (SmoothingCovariance.cov)."""
        return self._filter_call("vgpa_particle_covariance", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "mean": self._new(n_keep, self.D), "second": self._new(n_keep, self.D, self.D), "lineage_ess": self._new(self.n_obs + 1, fill=0.0)})

    def _ladder_input(self, levels):
        """levels of particle_marginals laid out for the C ABI: (B, D, L) float64 and L.  (L,) is every component's of every problem, (D, L)
        every problem's."""
        lev = np.asarray(levels, dtype=np.float64)
        if lev.ndim not in (1, 2, 3) or lev.size == 0:
            raise ValueError(f"levels has shape {lev.shape}, expected (L,), ({self.D}, L) or ({self.B}, {self.D}, L)")
        n_levels = lev.shape[-1]
        if lev.shape[:-1] not in ((), (self.D,), (self.B, self.D)):
            raise ValueError(f"levels has shape {lev.shape}, expected ({n_levels},), ({self.D}, {n_levels}) or ({self.B}, {self.D}, {n_levels})")
        if not 1 <= n_levels <= MAX_MARGINAL_LEVELS:
            raise ValueError(f"levels holds {n_levels} levels per component, expected 1 to {MAX_MARGINAL_LEVELS}")
        if lev.ndim == 1:
            lev = np.broadcast_to(lev, (self.D, n_levels))
        lev = _c64(per_problem(lev, self.B, self.D * n_levels)).reshape(self.B, self.D, n_levels)
        if not np.all(np.isfinite(lev)):
            raise ValueError("levels must be finite")
        if not np.all(lev[..., 1:] > lev[..., :-1]):
            p, d = np.argwhere(~np.all(lev[..., 1:] > lev[..., :-1], axis=-1))[0]
            raise ValueError(f"levels must be strictly increasing (problem {p}, component {d})")
        return lev, int(n_levels)

    def particle_marginals(self, n_paths, seed, levels, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None):
        """The smoothing marginals on the grid under particle_filter's genealogy (vgpa_particle_marginals): particle_moments' filter, descendant
        weights and second walk, which counts where that one sums.  levels: per problem and component a strictly increasing ladder of L <= 63
        finite levels, (B, D, L), or (D, L) or (L,) for every problem (and component); bin(x) = #{l: levels_l < x}.  Returns a dict: log_w,
        state, ess, resampled as particle_filter (bit for bit), mass (B, n_keep, D, L + 1) uint64: the sum of the lineages' integer weights per
        bin at the grid indices 0, stride, ..., exact and independent of any order of addition, q_final (B, n_paths) uint64:
        trunc(W 2^62) of the final weights, and lineage_ess as particle_moments (bit for bit)."""
        ladder = []      # (levels, L): made where _filter_call checks the entry's own inputs, read where it makes the outputs

        def inputs():
            ladder.extend(self._ladder_input(levels))
            return tuple(ladder)
        return self._filter_call("vgpa_particle_marginals", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "mass": self._new(n_keep, self.D, ladder[1] + 1, dtype=np.uint64), "q_final": self._new(n, dtype=np.uint64),
            "lineage_ess": self._new(self.n_obs + 1, fill=0.0)}, inputs=inputs)

    @staticmethod
    def _index_array(values, name, dtype):
        """a 1-D sequence of integers (a scalar is one of them) as a contiguous array of `dtype`"""
        v = np.asarray(values)
        if v.ndim == 0:
            v = v.reshape(1)
        if v.ndim != 1 or (v.size and v.dtype.kind not in "iu"):
            raise ValueError(f"{name} must be a 1-D sequence of integers")
        if v.size and (int(v.min()) < np.iinfo(dtype).min or int(v.max()) > np.iinfo(dtype).max):
            raise ValueError(f"{name} must fit into {np.iinfo(dtype).bits} bits")
        return np.ascontiguousarray(v, dtype=dtype)

    def particle_lag_covariance(self, n_paths, seed, anchors, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None):
        """The two-time moments of the smoothing law under particle_filter's genealogy (vgpa_particle_lag_covariance): the filter, the
        trajectory of every final slot as particle_paths(n_draw=n_paths, slots=arange(n_paths)) walks it -- kept on the device, B n_paths
        n_keep D doubles: the stride is the lever --, and their contraction with the normalised final weights W.  anchors: strictly
        increasing grid indices, each a multiple of stride, shared by the problems.  Returns a dict: log_w, state, ess, resampled as
        particle_filter (bit for bit), lineage_ess as particle_moments (bit for bit), mean (B, n_keep, D): sum W x(k), and cross
        (B, n_anchor, n_keep, D, D): sum W x(k) x(anchor)^T at the grid indices k = 0, stride, ..., on both sides of the anchor.  The
        covariance is cross - mean(k) mean(anchor)^T (SmoothingLagCovariance.cov)."""
        own = []      # (the anchors: made where _filter_call checks the entry's own inputs, read where it makes the outputs)

        def inputs():
            own.append(self._index_array(anchors, "anchors", np.int64))
            self._fit32(n_anchor=int(own[0].size))
            return int(own[0].size), (own[0] if own[0].size else None)
        return self._filter_call("vgpa_particle_lag_covariance", {"n_paths": n_paths, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "mean": self._new(n_keep, self.D), "cross": self._new(own[0].size, n_keep, self.D, self.D),
            "lineage_ess": self._new(self.n_obs + 1, fill=0.0)}, inputs=inputs)

    def path_cross_moments(self, paths, anchor_rows, weights=None):
        """The contraction of particle_lag_covariance alone on given trajectories (vgpa_path_cross_moments): paths (B, n, n_keep, D) -- or
        (n, n_keep, D) with B = 1 --, weights (B, n) or (n,) used as given (None: 1 / n each), anchor_rows: rows of the kept axis.  Returns
        (mean (B, n_keep, D), cross (B, n_anchor, n_keep, D, D)): sum_i W_i x_i(k) and sum_i W_i x_i(k) x_i(row)^T, every term
        fma(x_i(k)[a], W_i x_i(row)[b], .), the paths in increasing order.  Reads and writes nothing of the cached state."""
        pp = np.asarray(paths, dtype=np.float64)
        if pp.ndim == 3 and self.B == 1:
            pp = pp[None]
        if pp.ndim != 4 or pp.shape[0] != self.B or pp.shape[3] != self.D or pp.size == 0:
            raise ValueError(f"paths has shape {np.shape(paths)}, expected ({self.B}, n, n_keep, {self.D})")
        pp = _c64(pp)
        n, n_keep = pp.shape[1], pp.shape[2]
        ww = None
        if weights is not None:
            ww = np.asarray(weights, dtype=np.float64)
            if ww.size != self.B * n:
                raise ValueError(f"weights has {ww.size} entries, expected {self.B} x {n}")
            ww = _c64(ww.reshape(self.B, n))
        rows = self._index_array(anchor_rows, "anchor_rows", np.int32)
        self._fit32(n_paths=n, n_keep=n_keep, n_anchor=int(rows.size))
        mean, cross = self._new(n_keep, self.D), self._new(rows.size, n_keep, self.D, self.D)
        self._check(self._lib.vgpa_path_cross_moments(self._h, _ptr(pp), _ptr(ww), n, n_keep, int(rows.size), _ptr(rows) if rows.size else None,
                                                      _ptr(mean), _ptr(cross)))
        return mean, cross

    def particle_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None, slots=None):
        """n_draw whole smoothing trajectories per problem from particle_filter's genealogy (vgpa_particle_paths): the filter, the final
        slots (slots (B, n_draw) or (n_draw,), each in [0, n_paths); None: drawn from the final weights by systematic resampling, equally
        weighted), their slot in every stretch traced back through the ancestors, and one walk of the trajectories alone.  Returns a dict:
        log_w, state, ess, resampled as particle_filter (bit for bit), paths (B, n_draw, n_keep, D) at the grid indices 0, stride, ..., and
        slots (B, M + 1, n_draw) int32: the slot of every trajectory in every stretch (-1 beyond a problem's own count + 1)."""
        return self._smoothing_paths("vgpa_particle_paths", n_paths, seed, n_draw, stride, ess_fraction, x, x0, prior, slots)

    def particle_backward_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, prior=None, slots=None):
        """n_draw whole smoothing trajectories per problem by backward simulation through particle_filter's clouds
        (vgpa_particle_backward_paths): the arguments and the dict of particle_paths, the filter and the final slots the same; but at every
        observation where the cloud was resampled a trajectory does not follow its ancestor: it draws the slot it came from among all n
        particles, with probability proportional to filter weight times model transition density (Gumbel-max on the device, one launch).
        Where nothing was resampled (ess_fraction=0, n_paths=1) the result is particle_paths' bit for bit."""
        return self._smoothing_paths("vgpa_particle_backward_paths", n_paths, seed, n_draw, stride, ess_fraction, x, x0, prior, slots)

    def _smoothing_paths(self, entry, n_paths, seed, n_draw, stride, ess_fraction, x, x0, prior, slots):
        """what particle_paths and particle_backward_paths have of their own, one like the other"""
        return self._filter_call(entry, {"n_paths": n_paths, "n_draw": n_draw, "stride": stride}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "paths": self._new(k, n_keep, self.D), "slots": self._new(self.n_obs + 1, k, fill=-1, dtype=np.int32)}, slots=slots)

    def particle_conditional(self, ref, n_paths, seed, ess_fraction=0.5, x=None, x0=None, prior=None, history=False):
        """One sweep of particle Gibbs with ancestor sampling (vgpa_particle_conditional): particle_filter with slot 0 of every problem pinned
        to the reference trajectory ref (B, Np, D) (or (Np, D), shared) and weighted like any other slot, multinomial resampling, and the
        ancestor of the pinned slot drawn anew at every resampling.  Returns a dict: log_w, state, ess, resampled (and, history=True,
        ancestors and clouds) as particle_filter, of this run; trajectory (B, Np, D): the drawn trajectory, the next reference; slots
        (B, M + 1) int32: the slot it sat in during every stretch (0: that stretch is the reference's; -1 beyond a problem's count + 1)."""
        def reference():
            if ref is None:
                return (None,)
            rr = np.asarray(ref, dtype=np.float64)
            if rr.size not in (self.Np * self.D, self.B * self.Np * self.D):
                raise ValueError(f"ref has {rr.size} entries, expected {self.B} x {self.Np} x {self.D}")
            return (_c64(np.broadcast_to(rr.reshape(-1, self.Np, self.D), (self.B, self.Np, self.D))),)
        return self._filter_call("vgpa_particle_conditional", {"n_paths": n_paths}, seed, ess_fraction, x, x0, prior, lambda n, k, n_keep: {
            "trajectory": self._new(self.Np, self.D), "slots": self._new(self.n_obs + 1, fill=-1, dtype=np.int32)}, head=reference, history=bool(history))

    def particle_forecast(self, horizon, n_paths=None, seed=0, stride=1, n_draw=0, ess_fraction=0.5, x=None, x0=None, cloud=None, log_w=None,
                          index0=None, slots=None, prior=None):
        """A weighted cloud carried `horizon` steps past its grid index under the model SDE (vgpa_particle_forecast), on the device.
        cloud=None: the cloud is the final one of particle_filter(n_paths, seed, ess_fraction, x, x0, prior) at grid index Np - 1, taken
        from the device buffer it is in.  Else cloud (B, n, D) or (n, D), log_w (B, n) or (n,) (None: equal weights) and index0 (the
        absolute grid index of the cloud; None: Np - 1): no filter runs and the context need not have evaluated anything.  Step h draws at
        the absolute grid index index0 + h with the counter word of the particle's slot; the weights do not change.  n_draw members per
        problem are the trajectories of the slots `slots` ((B, n_draw) or (n_draw,); n_draw may then be left 0), or of slots drawn from the weights as particle_paths
        draws its final slots.  Returns a dict: moments (B, h_keep, 2, D): sum W x and sum W x^2 at the steps 0, stride, ... <= horizon,
        members (B, n_draw, h_keep, D), slots (B, n_draw) int32, state_end (B, n, D): the cloud at index0 + horizon, index0, and log_w,
        state: the cloud the forecast started from (behind the filter bit for bit particle_filter's, with its ess and resampled)."""
        horizon, stride, n_draw = int(horizon), int(stride), int(n_draw)
        if slots is not None and n_draw == 0:      # (given slots say how many they are)
            n_draw = int(np.shape(slots)[-1]) if np.ndim(slots) else 0
        given_cloud = cloud is not None
        if given_cloud:
            cl = np.asarray(cloud, dtype=np.float64)
            if cl.ndim < 2 or cl.shape[-1] != self.D or cl.size == 0:
                raise ValueError(f"cloud must be (B, n, {self.D}) or (n, {self.D})")
            cl = _c64(np.broadcast_to(cl.reshape((-1,) + cl.shape[-2:]), (self.B,) + cl.shape[-2:]))
            if n_paths is not None and int(n_paths) != cl.shape[1]:
                raise ValueError(f"n_paths = {n_paths}, but the cloud has {cl.shape[1]} particles")
            n_paths = cl.shape[1]
            lw = None if log_w is None else _c64(np.broadcast_to(np.asarray(log_w, dtype=np.float64).reshape(-1, n_paths), (self.B, n_paths)))
            k0 = self.Np - 1 if index0 is None else int(index0)
        else:
            if n_paths is None:
                raise ValueError("n_paths is needed where no cloud is given")
            if log_w is not None or index0 is not None:
                raise ValueError("log_w and index0 belong to a given cloud")
            cl, lw, k0 = None, None, self.Np - 1
        n_paths = int(n_paths)
        self._fit32(n_paths=n_paths, n_draw=n_draw, stride=stride, horizon=horizon, index0=k0)
        xx, s0, mu, tau = self._walk_inputs(x, x0, prior)
        n, k = max(n_paths, 0), max(n_draw, 0)
        given = self._slot_array(slots, k)
        h_keep = max(horizon, 0) // max(stride, 1) + 1
        out_lw, state, ess, flags = self._filter_outputs(n)
        moments, members = self._new(h_keep, 2, self.D), self._new(k, h_keep, self.D)
        table, state_end = self._new(k, fill=-1, dtype=np.int32), self._new(n, self.D)
        self._check(self._lib.vgpa_particle_forecast(self._h, _ptr(xx), _ptr(s0), n_paths, self._seed(seed), float(ess_fraction), _ptr(mu), _ptr(tau),
                                                     _ptr(cl), _ptr(lw), k0 if given_cloud else 0, horizon, stride, n_draw, _ptr(given), _ptr(out_lw),
                                                     _ptr(state), _ptr(ess), _ptr(flags), _ptr(moments), _ptr(members), _ptr(table), _ptr(state_end)))
        if given_cloud:
            out_lw, state, ess, flags = (self._new(n, fill=0.0) if lw is None else lw), cl, None, None
        return {"log_w": out_lw, "state": state, "ess": ess, "resampled": flags, "moments": moments, "members": members, "slots": table,
                "state_end": state_end, "index0": k0}

    def fetch(self, key):
        which = FETCH_IDS[key]
        if key in ("st", "psit", "Edf", "dEsde_ds"):
            out = np.empty(self._shape_m())
        elif key == "Esde_t":
            out = np.empty((self.B, self.Np))
        else:
            out = np.empty(self._shape_v())
        self._check(self._lib.vgpa_fetch(self._h, which, _ptr(out)))
        return self._squeeze(out)

    # ------------------------------------------------------------------ device-pointer path
    def alloc(self, count):
        return DeviceBuffer(self, count)

    def sweep_dev(self, x_buf, g_buf):
        f = np.empty(self.B)
        self._check(self._lib.vgpa_sweep_dev(self._h, x_buf.ptr, _ptr(f), g_buf.ptr))
        return float(f[0]) if self.B == 1 else f

    def free_energy_dev(self, x_buf):
        f = np.empty(self.B)
        self._check(self._lib.vgpa_free_energy_dev(self._h, x_buf.ptr, _ptr(f)))
        return float(f[0]) if self.B == 1 else f

    def sweep_enqueue(self, x_buf, g_buf):
        self._check(self._lib.vgpa_sweep_enqueue(self._h, x_buf.ptr, g_buf.ptr))

    def fetch_f(self):
        f = np.empty(self.B)
        self._check(self._lib.vgpa_fetch_f(self._h, _ptr(f)))
        return float(f[0]) if self.B == 1 else f

    def gradient_dev(self, g_buf):
        self._check(self._lib.vgpa_gradient_dev(self._h, g_buf.ptr))

    def release_x(self):
        """Tells the context that the device x of the last `*_dev` evaluation is about to be freed or overwritten."""
        self._check(self._lib.vgpa_release_x(self._h))

    # ------------------------------------------------------------------ device vector algebra (SCG)
    # Every vector is a DeviceBuffer of B segments; scalars are (B,) arrays, one per problem of the batch.
    def _seglen(self, buf):
        if buf.count % self.B:
            raise ValueError(f" vector of {buf.count} doubles does not split into {self.B} problems")
        return buf.count // self.B

    def _vreduce(self, fn, a, *b):
        out = np.empty(self.B)
        self._check(fn(self._h, a.ptr, *[v.ptr for v in b], self._seglen(a), _ptr(out)))
        return out

    def vdot(self, a, b):
        return self._vreduce(self._lib.vgpa_vec_dot, a, b)

    def vabsmax(self, a):
        return self._vreduce(self._lib.vgpa_vec_absmax, a)

    def vasum(self, a):
        return self._vreduce(self._lib.vgpa_vec_asum, a)

    def vaxpby(self, alpha, x, beta, y, out):
        """out = alpha*x + beta*y per problem (alpha, beta: scalars or (B,)); y=None drops the second term."""
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.B,)))
        be = None if y is None else np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.B,)))
        self._check(self._lib.vgpa_vec_axpby(self._h, self._seglen(x), _ptr(al), x.ptr,
                                             None if y is None else _ptr(be), None if y is None else y.ptr, out.ptr))

    def set_option(self, option, value):
        self._check(self._lib.vgpa_set_option(self._h, int(option), int(value)))

    def set_prior_energy(self, e0):
        """E0 = KL(q0||p0) used by the following objective calls (the reference recomputes it per call, variational.py:185)."""
        self._check(self._lib.vgpa_set_prior_energy(self._h, float(e0)))

    def set_problem_data(self, obs_t=None, obs_y=None, m0=None, s0=None, e0=None):
        """
        Gives every problem of the batch its own dataset: obs_t (B, M) grid indices, obs_y (B, M, D), m0 (B, D), s0 (B, D, D),
        e0 (B,).  Every array carries the leading batch axis, also at B = 1 or D = 1.  None keeps the shared value the context
        was created with; M is the context's observation count.  Drops the cached state.
        """
        B, M, D = self.B, self.n_obs, self.D
        t = _shaped(obs_t, (B, M), "obs_t", np.int64)
        y = _shaped(obs_y, (B, M, D), "obs_y")
        m = _shaped(m0, (B, D), "m0")
        s = _shaped(s0, (B, D, D), "s0")
        e = _shaped(e0, (B,), "e0")
        self._check(self._lib.vgpa_set_problem_data(self._h, _ptr(t), _ptr(y), _ptr(m), _ptr(s), _ptr(e)))

    def set_problem_params(self, theta=None, sigma=None):
        """
        Gives every problem of the batch its own drift parameters theta (B, n_theta) and system noise sigma (B, D, D) -- one
        parameter point per problem, e.g. a grid of (theta, sigma^2) over one dataset.  Both carry the leading batch axis, also at
        B = 1 or D = 1.  None keeps the shared value the context was created with; independent of set_problem_data.  Drops the
        cached state.  A non-positive-definite sigma row raises LinAlgError, a 1-D sigma <= 0 ValueError; the previous
        parameters then stay in force.
        """
        B, D = self.B, self.D
        t = _shaped(theta, (B, self.n_theta), "theta")
        s = _shaped(sigma, (B, D, D), "sigma")
        self._check(self._lib.vgpa_set_problem_params(self._h, _ptr(t), _ptr(s)))

    def set_problem_obs_model(self, n_obs=None, obs_noise=None, obs_h=None):
        """
        Gives every problem of the batch its own observation model: n_obs (B,) observation counts in [1, M] -- problem p then uses
        the first n_obs[p] entries of its obs_t / obs_y row and nothing behind them, so rows may be padded with anything --, obs_noise
        (B, D, D) and obs_h (B, D, D; not for 1-D models).  All carry the leading batch axis, also at B = 1 or D = 1.  None keeps the
        shared value the context was created with; M, the context's observation count, is the capacity of a row.  Drops the cached
        state.  A non-positive-definite obs_noise row raises LinAlgError, a count outside [1, M] or a 1-D obs_noise <= 0 ValueError;
        the previous model then stays in force.
        """
        B, D = self.B, self.D
        n = _shaped(n_obs, (B,), "n_obs", np.int64)
        n = None if n is None else np.ascontiguousarray(n, dtype=np.int32)
        r = _shaped(obs_noise, (B, D, D), "obs_noise")
        h = _shaped(obs_h, (B, D, D), "obs_h")
        self._check(self._lib.vgpa_set_problem_obs_model(self._h, _ptr(n), _ptr(r), _ptr(h)))

    @property
    def streaming(self):
        return bool(self._lib.vgpa_is_streaming(self._h))

    def _path(self):
        out = VgpaPath()
        self._check(self._lib.vgpa_path_info(self._h, byref(out)))
        return out

    def plan(self):
        """Which kernels this context's fused sweep runs (tests, diagnostics; read-only): the steppers `fwd` / `bwd` by name
        ("large_d", "lane", "wave", "mfma", "generic"), `helper_roles` as its count, every other field of the library's plan as a bool."""
        v, names = self._path(), {i: k for k, i in STEPPER_IDS.items()}
        plan = {k: names[getattr(v, k)] if k in ("fwd", "bwd") else bool(getattr(v, k)) for k in VgpaPath.PLAN}
        return dict(plan, helper_roles=int(v.helper_roles))

    def resident(self):
        """What the device buffers hold right now (tests, diagnostics; read-only): `cached` and `terms` as bools, `moments`
        ("row_major", "time_major"), `S` and `dEs` ("whole", "upper", "packed"), `bwd` ("none", "psi", "q")."""
        v = self._path()

        def name(ids, i):
            return {j: k for k, j in ids.items()}[i]
        return {"cached": bool(v.cached), "moments": name(MOMENTS_IDS, v.moments), "S": name(LAYOUT_IDS, v.S),
                "dEs": name(LAYOUT_IDS, v.dEs), "bwd": name(BWD_IDS, v.bwd_holds), "terms": bool(v.terms)}

    def synchronize(self):
        self._check(self._lib.vgpa_synchronize(self._h))

    def profile_begin(self):
        self._check(self._lib.vgpa_profile_begin(self._h))

    def profile_end(self):
        v = [c_double() for _ in range(4)]
        n = c_int64()
        self._check(self._lib.vgpa_profile_end(self._h, byref(v[0]), byref(v[1]), byref(v[2]), byref(v[3]), byref(n)))
        return dict(fwd_ms=v[0].value, energy_ms=v[1].value, bwd_ms=v[2].value, grad_ms=v[3].value, n_sweeps=n.value)
