"""rocket_path_amd -- MI355X-native batched interior-point trajectory step.

Only what the hot path needs: csrc/ (HIP kernels, the C ABI, the C++ Problem plug-in) and
this thin Python mirror of the same interface.  (The package directory uses '_' where the
project name has '-': Python identifiers cannot contain a hyphen.)
"""
from . import capi, problems  # noqa: F401
from .batch import Batch, Pipeline, solve_overlap, solve_overlap_stats  # noqa: F401
from .capi import (DTYPE_F32, DTYPE_F32_STATE, DTYPE_F64, ST_CONVERGED, ST_INFEASIBLE, ST_MAXITER, ST_NONFINITE, ST_STALLED, ST_WRONG_WAY,  # noqa: F401
                   VARIANT_F3, VARIANT_F4, RpError, device_count, device_id, load_library)


def __getattr__(name):
    # the torch layer (autograd.py) is imported on first use: everything else here works without importing torch
    if name in ("min_time_solve", "min_time_jacobian", "min_time_hessian", "trajectory_eval", "min_time_trajectory",
                "trajectory_crossing", "min_time_crossing", "trajectory_extrema", "min_time_extrema", "trajectory_integrals",
                "min_time_integrals", "trajectory_gap", "min_time_gap", "trajectory_tracking", "min_time_tracking",
                "trajectory_meeting", "min_time_meeting", "trajectory_separation", "synchronize_axes", "min_time_separation",
                "trajectory_contact", "min_time_contact", "fleet_pairs", "trajectory_fleet_separation", "min_time_fleet_separation",
                "trajectory_fleet_contact", "min_time_fleet_contact", "fleet_first_contact", "fleet_contact_candidates",
                "trajectory_fleet_reach", "cross_pairs", "static_fleet", "trajectory_cross_separation", "trajectory_cross_contact",
                "min_time_cross_separation", "min_time_cross_contact"):
        from . import autograd
        return getattr(autograd, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
