"""ctypes binding of the C ABI in include/rp_batch.h (lib/librp_batch.so).

This module is the only place Python touches the product library.  It never falls back to
anything: if the shared object is missing, or no HIP device is visible when a batch is
created, it raises.  The oracle under oracle/ is never imported from here.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librp_batch.so")

RP_OK = 0
ABI_VERSION = 7      # RP_ABI_VERSION of include/rp_batch.h this binding was written against
RP_ERR_INVALID, RP_ERR_DEVICE, RP_ERR_NOMEM, RP_ERR_UNSUPPORTED, RP_ERR_NO_DEVICE = 1, 2, 3, 4, 5
VARIANT_F3, VARIANT_F4 = 3, 4
DTYPE_F64, DTYPE_F32, DTYPE_F32_STATE = 0, 1, 2      # 2: fp32 state in HBM, fp64 arithmetic (include/rp_batch.h)
ST_CONVERGED, ST_MAXITER, ST_NONFINITE, ST_INFEASIBLE, ST_STALLED, ST_WRONG_WAY = 1, 2, 4, 8, 16, 32


class RpError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("rp_batch: status %d (%s)" % (status, text))
        self.status = status


class Params(ctypes.Structure):
    _fields_ = [("accel_limit", ctypes.c_double), ("mu_divisor", ctypes.c_double),
                ("boundary_fraction", ctypes.c_double), ("backtrack", ctypes.c_double),
                ("armijo", ctypes.c_double), ("max_backtracks", ctypes.c_int32), ("stall_window", ctypes.c_int32),
                ("mu_mode", ctypes.c_int32), ("mu_sigma_try", ctypes.c_double * 2),
                ("handoff_rounds", ctypes.c_int32), ("handoff_lanes", ctypes.c_int32)]


class Solution(ctypes.Structure):
    """rp_solution: one problem's answer, 32 bytes (as a numpy record: SOLUTION_FIELDS)."""
    _fields_ = [("vel1", ctypes.c_double), ("duration0", ctypes.c_double), ("duration1", ctypes.c_double),
                ("iters", ctypes.c_int32), ("status", ctypes.c_uint32)]


# numpy dtype description of an array of rp_solution records (np.dtype(SOLUTION_FIELDS), itemsize 32)
SOLUTION_FIELDS = [("vel1", "<f8"), ("duration0", "<f8"), ("duration1", "<f8"), ("iters", "<i4"), ("status", "<u4")]


class Reduction(ctypes.Structure):
    _fields_ = [("max_residual_sq", ctypes.c_double), ("max_gap", ctypes.c_double),
                ("n_converged", ctypes.c_double), ("total_steps", ctypes.c_double)]


_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)

# name -> (restype, argtypes); every symbol include/rp_batch.h declares
SIGNATURES = {
    "rp_version": (ctypes.c_char_p, []),
    "rp_abi_version": (ctypes.c_int, []),
    "rp_params_size": (ctypes.c_size_t, []),
    "rp_last_error": (ctypes.c_char_p, []),
    "rp_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "rp_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "rp_device_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "rp_params_default": (None, [ctypes.POINTER(Params)]),
    "rp_batch_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, _vp]),
    "rp_batch_destroy": (ctypes.c_int, [_vp]),
    "rp_batch_set_params": (ctypes.c_int, [_vp, ctypes.POINTER(Params)]),
    "rp_batch_get_params": (ctypes.c_int, [_vp, ctypes.POINTER(Params)]),
    "rp_batch_size": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t)]),
    "rp_batch_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "rp_batch_init_default": (ctypes.c_int, [_vp]),
    "rp_batch_init_stuck": (ctypes.c_int, [_vp]),
    "rp_batch_set_problems": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "rp_batch_set_problems_device": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "rp_batch_set_problems_vel": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_set_problems_vel_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_restart": (ctypes.c_int, [_vp]),
    "rp_batch_set_state": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_get_state": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_get_state_range": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
    "rp_batch_nudge": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double]),
    "rp_batch_step": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rp_batch_step_counted": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "rp_batch_solve": (ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int, ctypes.c_int]),
    "rp_batch_solve_launch": (ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int, ctypes.c_int]),
    "rp_batch_move_toward_feasibility": (ctypes.c_int, [_vp]),
    "rp_batch_get_iters": (ctypes.c_int, [_vp, _vp, _vp]),
    "rp_batch_solution_device": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_bind_solution": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_solution_vjp": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_solution_jvp": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_solution_jacobian": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_solution_hessian": (ctypes.c_int, [_vp, _vp, _vp]),
    "rp_batch_solution_vjp_vel": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_solution_jvp_vel": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_batch_solution_jacobian_vel": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_traffic_probe": (ctypes.c_int, [_vp]),
    "rp_batch_reduce": (ctypes.c_int, [_vp, ctypes.POINTER(Reduction)]),
    "rp_batch_reduce_device": (ctypes.c_int, [_vp, _vp]),
    "rp_batch_summary_device": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "rp_batch_summary_read": (ctypes.c_int, [_vp, ctypes.POINTER(Reduction)]),
    "rp_batch_sample": (ctypes.c_int, [_vp, _vp, _vp]),
    "rp_batch_sample_device": (ctypes.c_int, [_vp, _vp, _vp]),
    "rp_trajectory_eval": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, _vp, _vp]),
    "rp_trajectory_eval_vjp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, _vp, _vp,
                                              ctypes.POINTER(_vp), _vp]),
    "rp_trajectory_eval_jvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp),
                                              _vp, _vp, _vp, _vp]),
    "rp_trajectory_eval_hvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, _vp, _vp,
                                              ctypes.POINTER(_vp), _vp, ctypes.POINTER(_vp), _vp]),
    "rp_batch_trajectory_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "rp_trajectory_crossing": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, _vp]),
    "rp_batch_crossing_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, _vp]),
    "rp_trajectory_extrema": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp),
                                             ctypes.POINTER(_vp)]),
    "rp_batch_extrema_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "rp_trajectory_gap": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp,
                                         ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "rp_trajectory_meeting": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp,
                                             _vp, _vp, _vp, _vp]),
    "rp_trajectory_separation": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_vp),
                                                ctypes.POINTER(_vp), _vp, _vp, _vp, _vp, _vp]),
    "rp_trajectory_contact": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(_vp),
                                             ctypes.POINTER(_vp), _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_trajectory_fleet_separation": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                      ctypes.POINTER(_vp), _vp, _vp, _vp, _vp]),
    "rp_trajectory_fleet_contact": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                   ctypes.POINTER(_vp), _vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "rp_trajectory_cross_separation": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                      ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp, _vp]),
    "rp_trajectory_cross_contact": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                   ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, ctypes.c_int, _vp, _vp, _vp,
                                                   _vp]),
    "rp_trajectory_fleet_separation_staggered": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                                ctypes.POINTER(_vp), _vp, _vp, _vp, _vp, _vp, _vp]),
    "rp_trajectory_fleet_contact_staggered": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                             ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "rp_trajectory_fleet_reach": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                 ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "rp_trajectory_fleet_contact_culled_workspace": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                                    ctypes.POINTER(ctypes.c_size_t)]),
    "rp_trajectory_fleet_contact_culled": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                          ctypes.POINTER(_vp), _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                                          _vp, _vp, _vp]),
    "rp_trajectory_fleet_contact_candidates": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                              ctypes.POINTER(_vp), _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "rp_trajectory_fleet_reach_staggered": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                           ctypes.POINTER(_vp), _vp, _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "rp_trajectory_fleet_contact_staggered_culled_workspace": (ctypes.c_int, [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                                              ctypes.POINTER(ctypes.c_size_t)]),
    "rp_trajectory_fleet_contact_staggered_culled": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                                    ctypes.c_int, ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int, _vp, _vp, _vp,
                                                                    _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "rp_trajectory_fleet_contact_staggered_candidates": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                                        ctypes.c_int, ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int, _vp, _vp,
                                                                        _vp, ctypes.c_size_t, _vp]),
    "rp_trajectory_tracking": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp,
                                              _vp, ctypes.POINTER(_vp)]),
    "rp_trajectory_tracking_vjp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp,
                                                  _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp]),
    "rp_trajectory_tracking_jvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp,
                                                  _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp, ctypes.POINTER(_vp)]),
    "rp_trajectory_tracking_hvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp,
                                                  _vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp,
                                                  ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, _vp]),
    "rp_trajectory_integrals": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp)]),
    "rp_trajectory_integrals_vjp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp,
                                                   ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp]),
    "rp_trajectory_integrals_jvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp,
                                                   ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp)]),
    "rp_trajectory_integrals_hvp": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _vp,
                                                   ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp, ctypes.POINTER(_vp), _vp, _vp]),
    "rp_batch_integrals_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "rp_batch_sample_range": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _vp, _vp]),
    "rp_batch_constraints_range": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _vp]),
    "rp_batch_sync": (ctypes.c_int, [_vp]),
    "rp_batch_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "rp_solve_overlap_set": (ctypes.c_int, [ctypes.c_int]),
    "rp_solve_overlap_stats": (ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    "rp_batch_event_record": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rp_batch_event_elapsed_ms": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "rp_batch_field_ptr": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp)]),
    "rp_batch_slot_map": (ctypes.c_int, [_vp, _vp]),
    "rp_pipeline_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rp_pipeline_destroy": (ctypes.c_int, [_vp]),
    "rp_pipeline_set_params": (ctypes.c_int, [_vp, ctypes.POINTER(Params)]),
    "rp_pipeline_set_prep": (ctypes.c_int, [_vp, ctypes.c_int]),
    "rp_pipeline_submit": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_int64)]),
    "rp_pipeline_wait": (ctypes.c_int, [_vp, ctypes.c_int64]),
    "rp_pipeline_stream_wait": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp]),
    "rp_pipeline_batch": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(_vp)]),
}

_lib = None


def load_library(path=None):
    """Load librp_batch.so and bind every declared symbol.  Raises if the build is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RP_BATCH_LIB") or LIB_PATH      # RP_BATCH_LIB: a tuning build of the same ABI (A/B runs)
    if path is None and not os.path.exists(p) and os.path.exists("/opt/rocm/bin/hipcc"):
        # a checkout without built artefacts (they are git-ignored): compile, never substitute
        import subprocess
        subprocess.call(["make", "-C", os.path.join(_HERE, "csrc"), "all"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(p):
        raise RuntimeError(
            "HIP extension not built: %s is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rocket_path_amd/csrc`. There is no CPU fallback for this path." % p)
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.rp_abi_version() != ABI_VERSION or lib.rp_params_size() != ctypes.sizeof(Params):
        raise RuntimeError("%s was built for ABI revision %d (rp_params of %d bytes); this binding is revision %d (%d bytes): rebuild"
                           % (p, lib.rp_abi_version(), lib.rp_params_size(), ABI_VERSION, ctypes.sizeof(Params)))
    if path is None:
        _lib = lib
    return lib


def check(status):
    if status != RP_OK:
        lib = load_library()
        raise RpError(status, (lib.rp_last_error() or b"").decode() or lib.rp_status_string(status).decode())


def pointer_table(addresses):
    """Eight device addresses (ints; None / 0: NULL) as the `double *const [8]` tables of the rp_trajectory_* entries, in the order
    (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1); None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != 8:
        raise ValueError("a spline table has eight entries, got %d" % len(addresses))
    return (_vp * 8)(*[a if a else None for a in addresses])


def _trajectory(entry, device, stream, n, k, spline, d_tau, *rest):
    args = [pointer_table(a) if isinstance(a, (list, tuple)) else (ctypes.c_void_p(a) if a else None) for a in rest]
    check(getattr(load_library(), entry)(int(device), ctypes.c_void_p(stream) if stream else None, int(n), int(k), pointer_table(spline),
                                        ctypes.c_void_p(d_tau) if d_tau else None, *args))


def trajectory_eval(device, stream, n, k, spline, d_tau, d_pos=None, d_vel=None, d_acc=None):
    """rp_trajectory_eval on device addresses (ints; None / 0: NULL): `spline` the eight addresses of (pos0, pos1, pos2, vel0, vel2, vel1,
    duration0, duration1), d_tau and the outputs (n, k) float64.  Asynchronous on `stream` (None: the null stream)."""
    _trajectory("rp_trajectory_eval", device, stream, n, k, spline, d_tau, d_pos, d_vel, d_acc)


def trajectory_eval_vjp(device, stream, n, k, spline, d_tau, d_g_pos=None, d_g_vel=None, d_g_acc=None, spline_bar=None, d_tau_bar=None):
    """rp_trajectory_eval_vjp: upstream gradients in (None: zeros), `spline_bar` the eight output addresses (None entries: not wanted)."""
    _trajectory("rp_trajectory_eval_vjp", device, stream, n, k, spline, d_tau, d_g_pos, d_g_vel, d_g_acc,
                list(spline_bar) if spline_bar is not None else None, d_tau_bar)


def trajectory_eval_jvp(device, stream, n, k, spline, d_tau, spline_dot=None, d_tau_dot=None, d_pos_dot=None, d_vel_dot=None, d_acc_dot=None):
    """rp_trajectory_eval_jvp: `spline_dot` the eight tangent addresses (None entries: zeros), tangents of pos, vel, acc out."""
    _trajectory("rp_trajectory_eval_jvp", device, stream, n, k, spline, d_tau, list(spline_dot) if spline_dot is not None else None,
                d_tau_dot, d_pos_dot, d_vel_dot, d_acc_dot)


def trajectory_eval_hvp(device, stream, n, k, spline, d_tau, d_g_pos=None, d_g_vel=None, d_g_acc=None, spline_dot=None, d_tau_dot=None,
                        spline_bar_dot=None, d_tau_bar_dot=None):
    """rp_trajectory_eval_hvp: the derivative of trajectory_eval_vjp's outputs along (`spline_dot`, d_tau_dot) (None entries: zeros) at fixed
    upstream gradients; `spline_bar_dot` the eight output addresses (None entries: not wanted)."""
    _trajectory("rp_trajectory_eval_hvp", device, stream, n, k, spline, d_tau, d_g_pos, d_g_vel, d_g_acc,
                list(spline_dot) if spline_dot is not None else None, d_tau_dot,
                list(spline_bar_dot) if spline_bar_dot is not None else None, d_tau_bar_dot)


def trajectory_crossing(device, stream, n, k, spline, d_level, d_time, d_vel=None):
    """rp_trajectory_crossing: the first time in [0, duration0 + duration1] at which the spline is at each level (n, k), NaN where it never
    is, and (d_vel given) the velocity there.  Addresses as for trajectory_eval."""
    _trajectory("rp_trajectory_crossing", device, stream, n, k, spline, d_level, d_time, d_vel)


def extrema_table(addresses):
    """Four device addresses (ints; None / 0: NULL) as a `double *const [4]` table of the extrema entries, in the order (pos_min, pos_max,
    vel_min, vel_max); None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != 4:
        raise ValueError("an extrema table has four entries, got %d" % len(addresses))
    return (_vp * 4)(*[a if a else None for a in addresses])


def trajectory_extrema(device, stream, n, k, spline, d_lo=None, d_hi=None, value=None, time=None):
    """rp_trajectory_extrema: the extreme position and velocity of the spline over the windows [lo, hi] (n, k) clamped to
    [0, duration0 + duration1] (None / 0: -inf, +inf), and a time at which each is attained.  `value` and `time`: four addresses each in
    the order (pos_min, pos_max, vel_min, vel_max), None / 0 entries (or None for the table) not wanted.  Addresses as for
    trajectory_eval."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_extrema(int(device), vp(stream), int(n), int(k), pointer_table(spline), vp(d_lo), vp(d_hi),
                                               extrema_table(value), extrema_table(time)))


def gap_table(addresses):
    """Two device addresses (ints; None / 0: NULL) as a `double *const [2]` table of the gap entry, in the order (gap_min, gap_max); None
    gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != 2:
        raise ValueError("a gap table has two entries, got %d" % len(addresses))
    return (_vp * 2)(*[a if a else None for a in addresses])


def trajectory_gap(device, stream, n, k, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, value=None, time=None):
    """rp_trajectory_gap: the extreme gap pos_A(t) - pos_B(t - delay) between two splines over the windows [lo, hi] (n, k) clamped to their
    common time domain (None / 0: -inf, +inf, a delay of 0), and a time at which each is attained.  `spline_a`, `spline_b`: eight addresses
    each, as for trajectory_eval; `value` and `time`: two addresses each in the order (gap_min, gap_max), None / 0 entries (or None for the
    table) not wanted."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_gap(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b), vp(d_lo),
                                           vp(d_hi), vp(d_delay), gap_table(value), gap_table(time)))


def trajectory_meeting(device, stream, n, k, spline_a, spline_b, d_level=None, d_lo=None, d_hi=None, d_delay=None, d_time=None, d_relvel=None):
    """rp_trajectory_meeting: the first time in the windows [lo, hi] (n, k) clamped to the two splines' common time domain at which the gap
    pos_A(t) - pos_B(t - delay) is at `level` (None / 0: a level of 0, -inf, +inf, a delay of 0), NaN where it is not reached, and the
    closing velocity there (None / 0: not wanted).  `spline_a`, `spline_b`: eight addresses each, as for trajectory_eval."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_meeting(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b),
                                               vp(d_level), vp(d_lo), vp(d_hi), vp(d_delay), vp(d_time), vp(d_relvel)))


def axes_table(addresses, d):
    """8 d device addresses (ints; None / 0: NULL) as a `double *const [8 d]` table of rp_trajectory_separation, axis-major: axis c's eight in
    pointer_table's order at [8 c, 8 c + 8); None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if d < 1 or len(addresses) != 8 * d:
        raise ValueError("a table of %d axes has %d entries, got %d" % (d, 8 * d, len(addresses)))
    return (_vp * (8 * d))(*[a if a else None for a in addresses])


def trajectory_separation(device, stream, n, k, d, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, d_value=None, d_time=None):
    """rp_trajectory_separation: the least squared distance between two vehicles of `d` axes (1..3) over the windows [lo, hi] (n, k) clamped
    to the common time domain of their 2 d splines (None / 0: -inf, +inf, a delay of 0), and the time at which it is attained (None / 0:
    not wanted; not both).  `spline_a`, `spline_b`: 8 d addresses each, axis-major, each axis as for trajectory_eval."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d = int(d)
    if not 1 <= d <= 3:
        raise ValueError("trajectory_separation: d must be 1, 2 or 3, got %d" % d)
    check(load_library().rp_trajectory_separation(int(device), vp(stream), int(n), int(k), d, axes_table(spline_a, d), axes_table(spline_b, d),
                                                  vp(d_lo), vp(d_hi), vp(d_delay), vp(d_value), vp(d_time)))


def trajectory_contact(device, stream, n, k, d, spline_a, spline_b, d_level_sq, d_lo=None, d_hi=None, d_delay=None, d_time=None, d_rate=None):
    """rp_trajectory_contact: the first time in the windows [lo, hi] (n, k; trajectory_separation's clamping and None meanings) at which the
    squared distance between two vehicles of `d` axes (1..3) reaches `d_level_sq` (n, k, required), NaN where it does not (`d_time`,
    required), and the rate of change of the squared distance there (`d_rate`; None / 0: not wanted).  `spline_a`, `spline_b`: 8 d
    addresses each, axis-major, each axis as for trajectory_eval."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d = int(d)
    if not 1 <= d <= 3:
        raise ValueError("trajectory_contact: d must be 1, 2 or 3, got %d" % d)
    check(load_library().rp_trajectory_contact(int(device), vp(stream), int(n), int(k), d, axes_table(spline_a, d), axes_table(spline_b, d),
                                               vp(d_level_sq), vp(d_lo), vp(d_hi), vp(d_delay), vp(d_time), vp(d_rate)))


def _fleet_sizes(who, d, m):
    """(d, m) as ints, refused here where the C entry would refuse them"""
    d, m = int(d), int(m)
    if not 1 <= d <= 3:
        raise ValueError("%s: d must be 1, 2 or 3, got %d" % (who, d))
    if not 2 <= m <= 256:
        raise ValueError("%s: m must be 2..256 vehicles per scene, got %d" % (who, m))
    return d, m


def trajectory_fleet_separation(device, stream, n, m, k, d, fleet, d_lo=None, d_hi=None, d_value=None, d_time=None):
    """rp_trajectory_fleet_separation: trajectory_separation's two outputs, bit for bit with no delay, for every pair (i, j), i < j
    (lexicographic), of `n` scenes of `m` vehicles (2..256) of `d` axes (1..3) on one clock.  `fleet`: 8 d addresses, axis-major, each axis
    as for trajectory_eval, every array n m values with vehicle v of scene s at s m + v.  d_lo, d_hi: (n, k), the scene's windows for all
    its pairs (None / 0: -inf, +inf).  d_value, d_time: (n, m (m - 1) / 2, k) (None / 0: not wanted; not both)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes("trajectory_fleet_separation", d, m)
    check(load_library().rp_trajectory_fleet_separation(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), vp(d_lo), vp(d_hi),
                                                        vp(d_value), vp(d_time)))


def trajectory_fleet_contact(device, stream, n, m, k, d, fleet, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None, d_time=None, d_rate=None):
    """rp_trajectory_fleet_contact: trajectory_contact's two outputs, bit for bit with no delay, for every pair (i, j), i < j
    (lexicographic), of `n` scenes of `m` vehicles (2..256) of `d` axes (1..3) on one clock.  `fleet`, d_lo, d_hi as for
    trajectory_fleet_separation.  d_level_sq (required), squared distance: (n, k), one level for all pairs of a scene
    (level_per_pair 0), or (n, m (m - 1) / 2, k), 16-byte aligned (level_per_pair 1).  d_time (required), d_rate (None / 0: not wanted):
    (n, m (m - 1) / 2, k)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes("trajectory_fleet_contact", d, m)
    check(load_library().rp_trajectory_fleet_contact(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), vp(d_level_sq),
                                                     int(level_per_pair), vp(d_lo), vp(d_hi), vp(d_time), vp(d_rate)))


def _cross_sizes(who, d, m_a, m_b):
    """(d, m_a, m_b) as ints, refused here where the C entry would refuse them"""
    d, m_a, m_b = int(d), int(m_a), int(m_b)
    if not 1 <= d <= 3:
        raise ValueError("%s: d must be 1, 2 or 3, got %d" % (who, d))
    if not (1 <= m_a <= 32768 and 1 <= m_b <= 32768):
        raise ValueError("%s: m_a and m_b must be 1..32768 vehicles per scene, got %d and %d" % (who, m_a, m_b))
    return d, m_a, m_b


def trajectory_cross_separation(device, stream, n, m_a, m_b, k, d, fleet_a, fleet_b, d_lo=None, d_hi=None, d_value=None, d_time=None):
    """rp_trajectory_cross_separation: trajectory_separation's two outputs, bit for bit with no delay, for every vehicle i of fleet A
    (`m_a` of them, 1..32768) against every vehicle j of fleet B (`m_b`) of `n` scenes of `d` axes (1..3) on one clock; pair (i, j) at
    i m_b + j.  `fleet_a`, `fleet_b`: 8 d addresses each, axis-major, each axis as for trajectory_eval, every array n m_a (n m_b) values
    with vehicle v of scene s at s m_a + v (s m_b + v).  d_lo, d_hi: (n, k), the scene's windows for all its pairs (None / 0: -inf, +inf).
    d_value, d_time: (n, m_a m_b, k) (None / 0: not wanted; not both)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m_a, m_b = _cross_sizes("trajectory_cross_separation", d, m_a, m_b)
    check(load_library().rp_trajectory_cross_separation(int(device), vp(stream), int(n), m_a, m_b, int(k), d, axes_table(fleet_a, d),
                                                        axes_table(fleet_b, d), vp(d_lo), vp(d_hi), vp(d_value), vp(d_time)))


def trajectory_cross_contact(device, stream, n, m_a, m_b, k, d, fleet_a, fleet_b, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None,
                             d_time=None, d_rate=None):
    """rp_trajectory_cross_contact: trajectory_contact's two outputs, bit for bit with no delay, for the pairs, fleets and windows of
    trajectory_cross_separation.  d_level_sq (required), squared distance: (n, k), one level for all pairs of a scene (level_per_pair 0),
    or (n, m_a m_b, k), 16-byte aligned (level_per_pair 1).  d_time (required), d_rate (None / 0: not wanted): (n, m_a m_b, k)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m_a, m_b = _cross_sizes("trajectory_cross_contact", d, m_a, m_b)
    check(load_library().rp_trajectory_cross_contact(int(device), vp(stream), int(n), m_a, m_b, int(k), d, axes_table(fleet_a, d),
                                                     axes_table(fleet_b, d), vp(d_level_sq), int(level_per_pair), vp(d_lo), vp(d_hi),
                                                     vp(d_time), vp(d_rate)))


def trajectory_fleet_separation_staggered(device, stream, n, m, k, d, fleet, d_start, d_lo=None, d_hi=None, d_value=None, d_time=None,
                                         d_time_local=None):
    """rp_trajectory_fleet_separation_staggered: trajectory_fleet_separation with a start time per vehicle, d_start (n, m), required, on
    the scene's clock, on which d_lo, d_hi and d_time are.  Pair (i, j) is trajectory_separation's query, bit for bit, with the delay
    start_j - start_i over the window [lo - start_i, hi - start_i]; d_time_local is its time (vehicle i's clock), d_time that plus start_i.
    d_value, d_time, d_time_local: (n, m (m - 1) / 2, k) (None / 0: not wanted; not all three)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes("trajectory_fleet_separation_staggered", d, m)
    check(load_library().rp_trajectory_fleet_separation_staggered(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), vp(d_start),
                                                                  vp(d_lo), vp(d_hi), vp(d_value), vp(d_time), vp(d_time_local)))


def trajectory_fleet_contact_staggered(device, stream, n, m, k, d, fleet, d_start, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None, d_time=None,
                                       d_time_local=None, d_rate=None):
    """rp_trajectory_fleet_contact_staggered: trajectory_fleet_contact with a start time per vehicle, d_start (n, m), required: pair (i, j)
    is trajectory_contact's query, bit for bit, with the delay start_j - start_i over the window [lo - start_i, hi - start_i] at the same
    level; d_time_local is its time (vehicle i's clock), d_time that plus start_i, d_rate its rate.  The three outputs are
    (n, m (m - 1) / 2, k) (None / 0: not wanted; not all three)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes("trajectory_fleet_contact_staggered", d, m)
    check(load_library().rp_trajectory_fleet_contact_staggered(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), vp(d_start),
                                                               vp(d_level_sq), int(level_per_pair), vp(d_lo), vp(d_hi), vp(d_time),
                                                               vp(d_time_local), vp(d_rate)))


def _axis_outputs(addresses, d, name):
    """d device addresses (ints; None / 0: NULL) as a `double *const [d]` table; None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != d:
        raise ValueError("%s: a table of %d axes has %d entries, got %d" % (name, d, d, len(addresses)))
    return (_vp * d)(*[a if a else None for a in addresses])


def _fleet_reach(who, start, device, stream, n, m, k, d, fleet, d_lo, d_hi, d_min, d_max):
    """rp_<who> for the two reach mirrors; `start`: () or (d_start,), which follows the fleet's table"""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes(who, d, m)
    check(getattr(load_library(), "rp_" + who)(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), *map(vp, start), vp(d_lo),
                                               vp(d_hi), _axis_outputs(d_min, d, "d_min"), _axis_outputs(d_max, d, "d_max")))


def _culled_workspace(who, n, m, k, d):
    """rp_<who> for the two workspace mirrors"""
    d, m = _fleet_sizes(who, d, m)
    size = ctypes.c_size_t(0)
    check(getattr(load_library(), "rp_" + who)(int(n), m, int(k), d, ctypes.byref(size)))
    return size.value


def _fleet_broad_phase(who, start, outputs, copies, device, stream, n, m, k, d, fleet, d_level_sq, level_per_pair, d_lo, d_hi, d_workspace,
                       workspace_bytes):
    """rp_<who> for the culled and candidates mirrors; start: () or (d_start,); outputs: its times and rate; copies: d_kept, its d_list, d_count"""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    d, m = _fleet_sizes(who, d, m)
    check(getattr(load_library(), "rp_" + who)(int(device), vp(stream), int(n), m, int(k), d, axes_table(fleet, d), *map(vp, start),
                                               vp(d_level_sq), int(level_per_pair), vp(d_lo), vp(d_hi), *map(vp, outputs), vp(d_workspace),
                                               int(workspace_bytes), *map(vp, copies)))


def trajectory_fleet_reach(device, stream, n, m, k, d, fleet, d_lo=None, d_hi=None, d_min=None, d_max=None):
    """rp_trajectory_fleet_reach: per vehicle, axis and query the least and greatest position over the scene's window [lo, hi] (n, k;
    None / 0: -inf, +inf) -- trajectory_extrema's pos_min and pos_max of that spline and window, bit for bit.  `fleet` as for
    trajectory_fleet_separation.  d_min, d_max: d addresses each, axis c's to (n, m, k), 16-byte aligned (None / 0: not wanted; not all)."""
    _fleet_reach("trajectory_fleet_reach", (), device, stream, n, m, k, d, fleet, d_lo, d_hi, d_min, d_max)


def trajectory_fleet_contact_culled_workspace(n, m, k, d):
    """rp_trajectory_fleet_contact_culled_workspace: the bytes of workspace the culled entries need for (n, m, k, d)."""
    return _culled_workspace("trajectory_fleet_contact_culled_workspace", n, m, k, d)


def trajectory_fleet_contact_culled(device, stream, n, m, k, d, fleet, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None, d_time=None,
                                    d_rate=None, d_workspace=None, workspace_bytes=0, d_kept=None, d_list=None, d_count=None):
    """rp_trajectory_fleet_contact_culled: trajectory_fleet_contact's outputs, bit for bit, for the same first thirteen arguments, with the
    broad phase in front: pairs whose position boxes prove them further apart than the level in all k queries get their NaN without a
    search.  d_workspace: workspace_bytes >= trajectory_fleet_contact_culled_workspace(n, m, k, d) bytes, 16-byte aligned.  d_kept
    (n pairs bytes), d_list (n pairs uint32), d_count (one uint32): copies of the keep-flags, the list and its length (None / 0: none)."""
    _fleet_broad_phase("trajectory_fleet_contact_culled", (), (d_time, d_rate), (d_kept, d_list, d_count), device, stream, n, m, k, d, fleet,
                       d_level_sq, level_per_pair, d_lo, d_hi, d_workspace, workspace_bytes)


def trajectory_fleet_contact_candidates(device, stream, n, m, k, d, fleet, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None, d_workspace=None,
                                        workspace_bytes=0, d_kept=None):
    """rp_trajectory_fleet_contact_candidates: the broad phase of trajectory_fleet_contact_culled alone: d_kept (n pairs bytes, required),
    1 where the pair would go to the search.  The workspace as there."""
    _fleet_broad_phase("trajectory_fleet_contact_candidates", (), (), (d_kept,), device, stream, n, m, k, d, fleet, d_level_sq, level_per_pair,
                       d_lo, d_hi, d_workspace, workspace_bytes)


def trajectory_fleet_reach_staggered(device, stream, n, m, k, d, fleet, d_start, d_lo=None, d_hi=None, d_min=None, d_max=None):
    """rp_trajectory_fleet_reach_staggered: trajectory_fleet_reach with a start time per vehicle, d_start (n, m), required: vehicle v's
    window is [lo - start_v, hi - start_v], on its own clock."""
    _fleet_reach("trajectory_fleet_reach_staggered", (d_start,), device, stream, n, m, k, d, fleet, d_lo, d_hi, d_min, d_max)


def trajectory_fleet_contact_staggered_culled_workspace(n, m, k, d):
    """rp_trajectory_fleet_contact_staggered_culled_workspace: the bytes of workspace the staggered culled entries need for (n, m, k, d)."""
    return _culled_workspace("trajectory_fleet_contact_staggered_culled_workspace", n, m, k, d)


def trajectory_fleet_contact_staggered_culled(device, stream, n, m, k, d, fleet, d_start, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None,
                                              d_time=None, d_time_local=None, d_rate=None, d_workspace=None, workspace_bytes=0, d_kept=None,
                                              d_list=None, d_count=None):
    """rp_trajectory_fleet_contact_staggered_culled: trajectory_fleet_contact_staggered's outputs, bit for bit, for the same first fifteen
    arguments, with the broad phase in front: a pair each of whose k queries is refused (no common time in the window) or box-far gets its
    NaN without a search.  The workspace (trajectory_fleet_contact_staggered_culled_workspace), d_kept, d_list and d_count as
    trajectory_fleet_contact_culled's."""
    _fleet_broad_phase("trajectory_fleet_contact_staggered_culled", (d_start,), (d_time, d_time_local, d_rate), (d_kept, d_list, d_count), device,
                       stream, n, m, k, d, fleet, d_level_sq, level_per_pair, d_lo, d_hi, d_workspace, workspace_bytes)


def trajectory_fleet_contact_staggered_candidates(device, stream, n, m, k, d, fleet, d_start, d_level_sq, level_per_pair=0, d_lo=None, d_hi=None,
                                                  d_workspace=None, workspace_bytes=0, d_kept=None):
    """rp_trajectory_fleet_contact_staggered_candidates: the broad phase of trajectory_fleet_contact_staggered_culled alone: d_kept
    (n pairs bytes, required), 1 where the pair would go to the search.  The workspace as there."""
    _fleet_broad_phase("trajectory_fleet_contact_staggered_candidates", (d_start,), (), (d_kept,), device, stream, n, m, k, d, fleet, d_level_sq,
                       level_per_pair, d_lo, d_hi, d_workspace, workspace_bytes)


def tracking_table(addresses):
    """Three device addresses (ints; None / 0: NULL) as a `double *const [3]` table of the tracking entries, in the order (gap_int, gap_sq,
    relvel_sq); None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != 3:
        raise ValueError("a tracking table has three entries, got %d" % len(addresses))
    return (_vp * 3)(*[a if a else None for a in addresses])


def trajectory_tracking(device, stream, n, k, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, value=None):
    """rp_trajectory_tracking: the integrals of D, D^2 and (dD/dt)^2, D(t) = pos_A(t) - pos_B(t - delay), over the windows [lo, hi] (n, k)
    clamped to the two splines' common time domain (None / 0: -inf, +inf, a delay of 0).  `spline_a`, `spline_b`: eight addresses each, as
    for trajectory_eval; `value`: three addresses in the order (gap_int, gap_sq, relvel_sq), None / 0 entries not wanted."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_tracking(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b),
                                                vp(d_lo), vp(d_hi), vp(d_delay), tracking_table(value)))


def trajectory_tracking_vjp(device, stream, n, k, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, g=None, spline_a_bar=None,
                            spline_b_bar=None, d_lo_bar=None, d_hi_bar=None, d_delay_bar=None):
    """rp_trajectory_tracking_vjp: `g` the three upstream gradients (None entries, or None: zeros), `spline_a_bar`, `spline_b_bar` the eight
    output addresses each and d_lo_bar, d_hi_bar, d_delay_bar (n, k) (None: not wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_tracking_vjp(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b),
                                                    vp(d_lo), vp(d_hi), vp(d_delay), tracking_table(g), pointer_table(spline_a_bar),
                                                    pointer_table(spline_b_bar), vp(d_lo_bar), vp(d_hi_bar), vp(d_delay_bar)))


def trajectory_tracking_jvp(device, stream, n, k, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, spline_a_dot=None, spline_b_dot=None,
                            d_lo_dot=None, d_hi_dot=None, d_delay_dot=None, value_dot=None):
    """rp_trajectory_tracking_jvp: `spline_a_dot`, `spline_b_dot` the eight tangent addresses each and d_lo_dot, d_hi_dot, d_delay_dot (None:
    zeros), `value_dot` the three output addresses (None entries: not wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_tracking_jvp(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b),
                                                    vp(d_lo), vp(d_hi), vp(d_delay), pointer_table(spline_a_dot), pointer_table(spline_b_dot),
                                                    vp(d_lo_dot), vp(d_hi_dot), vp(d_delay_dot), tracking_table(value_dot)))


def trajectory_tracking_hvp(device, stream, n, k, spline_a, spline_b, d_lo=None, d_hi=None, d_delay=None, g=None, spline_a_dot=None,
                            spline_b_dot=None, d_lo_dot=None, d_hi_dot=None, d_delay_dot=None, spline_a_bar_dot=None, spline_b_bar_dot=None,
                            d_lo_bar_dot=None, d_hi_bar_dot=None, d_delay_bar_dot=None):
    """rp_trajectory_tracking_hvp: the derivative of trajectory_tracking_vjp's outputs along (`spline_a_dot`, `spline_b_dot`, d_lo_dot,
    d_hi_dot, d_delay_dot) (None entries: zeros) at fixed upstream gradients `g`; `spline_a_bar_dot`, `spline_b_bar_dot` the eight output
    addresses each and d_lo_bar_dot, d_hi_bar_dot, d_delay_bar_dot (None: not wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_tracking_hvp(int(device), vp(stream), int(n), int(k), pointer_table(spline_a), pointer_table(spline_b),
                                                    vp(d_lo), vp(d_hi), vp(d_delay), tracking_table(g), pointer_table(spline_a_dot),
                                                    pointer_table(spline_b_dot), vp(d_lo_dot), vp(d_hi_dot), vp(d_delay_dot),
                                                    pointer_table(spline_a_bar_dot), pointer_table(spline_b_bar_dot), vp(d_lo_bar_dot),
                                                    vp(d_hi_bar_dot), vp(d_delay_bar_dot)))


def integrals_table(addresses):
    """Four device addresses (ints; None / 0: NULL) as a `double *const [4]` table of the integrals entries, in the order (pos_int,
    distance, vel_sq, acc_sq); None gives a NULL table."""
    if addresses is None:
        return None
    addresses = list(addresses)
    if len(addresses) != 4:
        raise ValueError("an integrals table has four entries, got %d" % len(addresses))
    return (_vp * 4)(*[a if a else None for a in addresses])


def trajectory_integrals(device, stream, n, k, spline, d_lo=None, d_hi=None, value=None):
    """rp_trajectory_integrals: the integrals of pos, |vel|, vel^2 and acc^2 over the windows [lo, hi] (n, k) clamped to
    [0, duration0 + duration1] (None / 0: -inf, +inf).  `value`: four addresses in the order (pos_int, distance, vel_sq, acc_sq), None / 0
    entries not wanted.  Addresses as for trajectory_eval."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_integrals(int(device), vp(stream), int(n), int(k), pointer_table(spline), vp(d_lo), vp(d_hi),
                                                 integrals_table(value)))


def trajectory_integrals_vjp(device, stream, n, k, spline, d_lo=None, d_hi=None, g=None, spline_bar=None, d_lo_bar=None, d_hi_bar=None):
    """rp_trajectory_integrals_vjp: `g` the four upstream gradients (None entries, or None: zeros), `spline_bar` the eight output addresses
    and d_lo_bar, d_hi_bar (n, k) (None: not wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_integrals_vjp(int(device), vp(stream), int(n), int(k), pointer_table(spline), vp(d_lo), vp(d_hi),
                                                     integrals_table(g), pointer_table(spline_bar), vp(d_lo_bar), vp(d_hi_bar)))


def trajectory_integrals_jvp(device, stream, n, k, spline, d_lo=None, d_hi=None, spline_dot=None, d_lo_dot=None, d_hi_dot=None, value_dot=None):
    """rp_trajectory_integrals_jvp: `spline_dot` the eight tangent addresses and d_lo_dot, d_hi_dot (None: zeros), `value_dot` the four
    output addresses (None entries: not wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_integrals_jvp(int(device), vp(stream), int(n), int(k), pointer_table(spline), vp(d_lo), vp(d_hi),
                                                     pointer_table(spline_dot), vp(d_lo_dot), vp(d_hi_dot), integrals_table(value_dot)))


def trajectory_integrals_hvp(device, stream, n, k, spline, d_lo=None, d_hi=None, g=None, spline_dot=None, d_lo_dot=None, d_hi_dot=None,
                             spline_bar_dot=None, d_lo_bar_dot=None, d_hi_bar_dot=None):
    """rp_trajectory_integrals_hvp: the derivative of trajectory_integrals_vjp's outputs along (`spline_dot`, d_lo_dot, d_hi_dot) (None
    entries: zeros) at fixed upstream gradients `g`; `spline_bar_dot` the eight output addresses and d_lo_bar_dot, d_hi_bar_dot (None: not
    wanted)."""
    vp = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    check(load_library().rp_trajectory_integrals_hvp(int(device), vp(stream), int(n), int(k), pointer_table(spline), vp(d_lo), vp(d_hi),
                                                     integrals_table(g), pointer_table(spline_dot), vp(d_lo_dot), vp(d_hi_dot),
                                                     pointer_table(spline_bar_dot), vp(d_lo_bar_dot), vp(d_hi_bar_dot)))


OVERLAP_OFF, OVERLAP_AUTO, OVERLAP_ALWAYS = 0, 1, 2      # rp_solve_overlap_set's modes


def solve_overlap_set(mode):
    """rp_solve_overlap_set: 0 = every call on the batch's stream, 1 = back-to-back fused solves of batches that share a stream overlap on
    an auxiliary stream (the default; batches of 65,536 problems or more), 2 = every eligible solve whatever its size.  Process-wide."""
    check(load_library().rp_solve_overlap_set(int(mode)))


def solve_overlap_stats():
    """rp_solve_overlap_stats as a dict: solves sent to the auxiliary stream, eligible solves kept on the caller's stream, joins enqueued,
    solves excluded by the eligibility list (counted since the library was loaded)."""
    out = (ctypes.c_ulonglong * 4)()
    check(load_library().rp_solve_overlap_stats(out))
    return {"aux": int(out[0]), "kept": int(out[1]), "joins": int(out[2]), "excluded": int(out[3])}


def device_count():
    """Number of visible HIP devices (0 when there is none)."""
    n = ctypes.c_int(0)
    load_library().rp_device_count(ctypes.byref(n))
    return n.value


def device_id(device):
    """'pci <bus id> uuid <hex>' of HIP device `device` (rp_device_id)."""
    buf = ctypes.create_string_buffer(128)
    check(load_library().rp_device_id(int(device), buf, 128))
    return buf.value.decode()
