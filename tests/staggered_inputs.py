"""The inputs of tests/staggered_gpu_cases.py and the conditions they are held to, in numpy alone, so that the conditions can be measured
without a device: per-vehicle start times, the windows over a scene's span, the pair entry's view of a staggered
fleet, and the shares the section quotes."""
import numpy as np

SPREAD = 2.0      # the starts of a scene are spread over this many of its shortest total time


def pairs_of(m):
    first, second = np.triu_indices(m, 1)
    return first, second


def totals(fleet):
    """(n, m, d): every spline's total time"""
    return np.stack([axis[6] + axis[7] for axis in fleet], axis=2)


def starts_of(fleet, spread=SPREAD):
    """default_rng(2700 + m).uniform(0, 1, (n, m)) * spread * the smallest total time of the scene's splines"""
    n, m = fleet[0][0].shape
    shortest = totals(fleet).min(axis=(1, 2))[:, None]
    return np.ascontiguousarray(np.random.default_rng(2700 + m).uniform(0, 1, (n, m)) * spread * shortest)


def scene_windows(fleet, start, k, seed):
    """Section 18's windows over each scene's span [min start, max (start + T)]: columns 0 and 1 (-inf, +inf), the others the sorted pair
    of two U(-0.1, 1.1) draws across the span: (lo, hi), (n, k)."""
    n, m = start.shape
    rng = np.random.default_rng(seed)
    S = start.min(axis=1)[:, None]
    E = (start[:, :, None] + totals(fleet)).max(axis=(1, 2))[:, None]
    draws = np.sort(rng.uniform(-0.1, 1.1, (n, k, 2)), axis=2)
    lo, hi = S + draws[:, :, 0] * (E - S), S + draws[:, :, 1] * (E - S)
    lo[:, :2], hi[:, :2] = -np.inf, np.inf
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def gathered(fleet, start, lo, hi, k=None):
    """The pair entry's inputs: A, B (d lists of eight arrays of n pairs values), lo', hi', delay (n pairs, k) and the first vehicle's start
    (n, pairs, 1).  A window end of None is the infinity before the subtraction."""
    n, m = start.shape
    first, second = pairs_of(m)
    k = k if k is not None else next(x for x in (lo, hi) if x is not None).shape[1]
    a = [[np.ascontiguousarray(x[:, first].reshape(-1)) for x in axis] for axis in fleet]
    b = [[np.ascontiguousarray(x[:, second].reshape(-1)) for x in axis] for axis in fleet]
    s_i, s_j = start[:, first][:, :, None], start[:, second][:, :, None]
    lo = lo if lo is not None else np.full((n, k), -np.inf)
    hi = hi if hi is not None else np.full((n, k), np.inf)
    with np.errstate(all="ignore"):
        delay = np.ascontiguousarray(np.broadcast_to(s_j - s_i, (n, len(first), k)).reshape(-1, k))
        lo_p = np.ascontiguousarray((lo[:, None, :] - s_i).reshape(-1, k))
        hi_p = np.ascontiguousarray((hi[:, None, :] - s_i).reshape(-1, k))
    return a, b, lo_p, hi_p, delay, s_i


def input_shares(fleet, start):
    """(the share of the pairs with a common time, the share with delay > 0): on the inputs alone"""
    n, m = start.shape
    first, second = pairs_of(m)
    shortest = totals(fleet).min(axis=2)
    delay = start[:, second] - start[:, first]
    common = np.maximum(delay, 0.0) <= np.minimum(shortest[:, first], delay + shortest[:, second])
    return float(common.mean()), float((delay > 0).mean())


def share_inside(fleet, start, lo, hi, value, local):
    """of the finite queries, the share whose local time is strictly inside the clamped window: on the pair entry's outputs"""
    n, m = start.shape
    first, second = pairs_of(m)
    shortest = totals(fleet).min(axis=2)
    s_i = start[:, first][:, :, None]
    delay = (start[:, second] - start[:, first])[:, :, None]
    S = np.maximum(delay, 0.0)
    E = np.minimum(shortest[:, first], (start[:, second] - start[:, first]) + shortest[:, second])[:, :, None]
    finite = np.isfinite(value)
    with np.errstate(all="ignore"):
        within = finite & (local > np.maximum(lo[:, None, :] - s_i, S)) & (local < np.minimum(hi[:, None, :] - s_i, E))
    return float(within.sum() / max(finite.sum(), 1)), float(finite.mean())
