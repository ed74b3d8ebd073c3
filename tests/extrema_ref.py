"""Test-side restatements of the position and velocity extremes (rp_trajectory_extrema, csrc/trajectory.hip), on
top of tests/trajectory_ref.py and tests/crossing_ref.py: a spline is its list of eight arrays, a window two (n, k) arrays lo and hi
(None: -inf / +inf).  The four outputs are in the entry's order, NAMES = (pos_min, pos_max, vel_min, vel_max).

    candidates_ld    the definition's candidate list in longdouble with true divisions: per quantity the times (n, k) in time order, whether
                     each takes part, and the value there (trajectory_ref.forward_ld at that time)
    extrema_ld       the definition: the strict walk over candidates_ld; (values, times), four (n, k) longdouble arrays each
    extrema_f64      the kernel's rule in float64, operation for operation (the staged stationary times through the kernel's quadratic
                     formula, values through trajectory_ref.forward_f64 at the global times; 1 / h is numpy's division where the kernel has
                     its refined reciprocal, so it restates the rule, not the bits)
    classes          the class of each returned time by equality, in the torch layer's priority: LO, HI, END, KNOT, interior
    derivative_ld / derivative_jvp_ld
                     the documented routing on trajectory_ref.vjp_ld / jvp_ld at the returned times
    runner_up_gap    per query and output, how far the best candidate beats every candidate at a different time, in units of the scale
    windows          the test windows; knot_cases the hand-made family whose extremes sit on the knot
"""
import os

import numpy as np

import crossing_ref as cr
import trajectory_ref as tr

LD = np.longdouble
NAMES = ("pos_min", "pos_max", "vel_min", "vel_max")
LO, HI, END, KNOT, INTERIOR, NONE = 0, 1, 2, 3, 4, 5


def _window(spline, lo, hi, k=None):
    """(lo, hi) as float64 (n, k) arrays: None is -inf / +inf, both None one whole-spline window per problem."""
    n = len(spline[0])
    given = lo if lo is not None else hi
    shape = (n, 1 if k is None else k) if given is None else np.shape(given)
    lo = np.full(shape, -np.inf) if lo is None else np.asarray(lo)
    hi = np.full(shape, np.inf) if hi is None else np.asarray(hi)
    return lo, hi


def _stationary(spline, T):
    """Per problem, (n, 1) columns of type T: the four stationary times of pos (two per segment, the earlier first, NaN: none) and the two
    of vel, all global; duration0; and the total time, the FLOAT64 sum in either type."""
    segs, d0 = cr._segments(spline, T, T is LD)
    nan = T(np.nan)
    tp, tv = [], []
    with np.errstate(all="ignore"):
        for g, (_, va, acc0, jrk0, h) in enumerate(segs):
            a, b, c = jrk0 * T(0.5), acc0, va
            disc = b * b - T(4) * (a * c)
            ok = disc >= 0
            q = T(-0.5) * (b + np.copysign(np.sqrt(np.where(ok, disc, T(0))), b))
            r0 = np.where(ok & (a != 0), q / np.where(a != 0, a, T(1)), nan)
            r1 = np.where(ok, c / q, nan)
            r0 = np.where((r0 > 0) & (r0 < h), r0, nan)
            r1 = np.where((r1 > 0) & (r1 < h), r1, nan)
            swap = (r1 < r0) | np.isnan(r0)
            first, second = np.where(swap, r1, r0), np.where(swap, r0, r1)
            s = np.where(jrk0 != 0, -acc0 / np.where(jrk0 != 0, jrk0, T(1)), nan)
            s = np.where((s > 0) & (s < h), s, nan)
            off = d0 if g else T(0) * d0
            tp += [off + first, off + second]
            tv += [off + s]
        p = tr._columns(spline, np.float64)
        total = (p[6] + p[7]).astype(T)
    return tp, tv, d0, total


def _candidates(spline, lo, hi, T):
    forward = tr.forward_ld if T is LD else tr.forward_f64
    lo, hi = _window(spline, lo, hi)
    lo, hi = lo.astype(T), hi.astype(T)
    tp, tv, d0, total = _stationary(spline, T)
    with np.errstate(all="ignore"):
        a = np.where(lo > 0, lo, np.where(np.isnan(lo), lo, T(0)))
        b = np.where(hi < total, hi, np.where(np.isnan(hi), hi, np.broadcast_to(total, hi.shape)))
        ok = a <= b
        knot = ok & (a <= d0) & (d0 <= b)
        inside = lambda t: ok & (a < t) & (t < b)      # noqa: E731
        wide = lambda t: np.broadcast_to(t, a.shape)      # noqa: E731
        times_p = [a, wide(tp[0]), wide(tp[1]), wide(d0), wide(tp[2]), wide(tp[3]), b]
        valid_p = [ok, inside(tp[0]), inside(tp[1]), knot, inside(tp[2]), inside(tp[3]), ok]
        times_v = [a, wide(tv[0]), wide(d0), wide(tv[1]), b]
        valid_v = [ok, inside(tv[0]), knot, inside(tv[1]), ok]
        value_p = [forward(spline, np.where(v, t, T(0)))[0] for t, v in zip(times_p, valid_p)]
        value_v = [forward(spline, np.where(v, t, T(0)))[1] for t, v in zip(times_v, valid_v)]
    return (times_p, valid_p, value_p), (times_v, valid_v, value_v)


def candidates_ld(spline, lo=None, hi=None):
    """((times, valid, values) of pos, the same of vel): lists of (n, k) arrays, in time order -- a, the stationary points strictly inside
    (a, b), the knot if a <= duration0 <= b (between the segments' stationary points), b."""
    return _candidates(spline, lo, hi, LD)


def _walk(times, valid, values, T):
    """The strict walk: (min value, min time, max value, max time); the earliest among equals, a NaN never."""
    shape = times[0].shape
    nan = np.full(shape, np.nan, dtype=T)
    lo_v, lo_t, hi_v, hi_t = nan.copy(), nan.copy(), nan.copy(), nan.copy()
    with np.errstate(all="ignore"):
        for t, ok, v in zip(times, valid, values):
            less = ok & ((v < lo_v) | (np.isnan(lo_v) & ~np.isnan(v)))
            more = ok & ((v > hi_v) | (np.isnan(hi_v) & ~np.isnan(v)))
            lo_v, lo_t = np.where(less, v, lo_v), np.where(less, t, lo_t)
            hi_v, hi_t = np.where(more, v, hi_v), np.where(more, t, hi_t)
    return lo_v, lo_t, hi_v, hi_t


def _extrema(spline, lo, hi, T):
    pos, vel = _candidates(spline, lo, hi, T)
    p, v = _walk(*pos, T), _walk(*vel, T)
    return [p[0], p[2], v[0], v[2]], [p[1], p[3], v[1], v[3]]


def extrema_ld(spline, lo=None, hi=None):
    """(values, times): four (n, k) longdouble arrays each, NAMES' order; NaN where the clamped window is empty."""
    return _extrema(spline, lo, hi, LD)


def extrema_f64(spline, lo=None, hi=None):
    """The same by the kernel's rule in float64."""
    return _extrema(spline, lo, hi, np.float64)


def runner_up_gap(spline, lo=None, hi=None):
    """Four (n, k) float64 arrays: by how much of the scale (trajectory_ref.scales: pos for the first two, vel for the others) the best
    candidate of the definition beats every candidate at a different time; inf where there is no other, NaN where the window is empty."""
    pos, vel = candidates_ld(spline, lo, hi)
    sc = tr.scales(spline)
    out = []
    for (times, valid, values), scale in ((pos, sc[0]), (vel, sc[1])):
        lo_v, lo_t, hi_v, hi_t = _walk(times, valid, values, LD)
        for sign, best_v, best_t in ((1, lo_v, lo_t), (-1, hi_v, hi_t)):
            gap = np.full(best_v.shape, np.inf, dtype=LD)
            with np.errstate(all="ignore"):
                for t, ok, v in zip(times, valid, values):
                    other = ok & (t != best_t) & ~np.isnan(v)
                    gap = np.where(other, np.minimum(gap, sign * (v - best_v)), gap)
            out.append(np.where(np.isnan(best_v), np.nan, np.asarray(gap / scale, dtype=np.float64)))
    return out


# ---------------------------------------------------------------- derivatives: the routing
def classes(spline, lo, hi, time):
    """The class of each returned time (n, k): LO where time == lo, else HI where time == hi, else END where time == duration0 +
    duration1 (the float64 sum), else KNOT where time == duration0, else INTERIOR; NONE where it is NaN."""
    lo, hi = _window(spline, lo, hi, np.shape(time)[1])
    p = tr._columns(spline, np.float64)
    d0, total = p[6], p[6] + p[7]
    t = np.asarray(time)
    out = np.full(t.shape, INTERIOR)
    with np.errstate(all="ignore"):
        for cls, ref in ((KNOT, d0), (END, total), (HI, hi), (LO, lo)):      # the last one written wins: the priority, backwards
            out = np.where(t == ref, cls, out)
    return np.where(np.isnan(t.astype(np.float64)), NONE, out)


def _side_by_side(spline, lo, hi, times, values):
    k = np.shape(times[0])[1]
    tau = np.concatenate([np.asarray(t, dtype=LD) for t in times], axis=1)
    missing = np.isnan(tau) | np.isnan(np.concatenate([np.asarray(v, dtype=LD) for v in values], axis=1))
    cls = np.concatenate([classes(spline, lo, hi, t) for t in times], axis=1)
    cls = np.where(missing, NONE, cls)
    return k, np.where(missing, LD(0), tau), missing, cls


def derivative_ld(spline, lo, hi, times, values, g, vjp=tr.vjp_ld):
    """Reverse mode in longdouble (vjp=trajectory_ref.vjp_f64: with the evaluator's float64 restatement) at the times given: (eight spline gradients, lo_bar (n, k), hi_bar (n, k)) for the upstream gradients g
    (four (n, k) arrays) on the four values.  One evaluator VJP at the four time arrays side by side, g_pos = [g0 | g1 | 0 | 0],
    g_vel = [0 | 0 | g2 | g3], 0 where the value is NaN; tau_bar goes to lo_bar (LO), hi_bar (HI), duration0_bar and duration1_bar
    (END), duration0_bar (KNOT), nowhere (interior)."""
    k, tau, missing, cls = _side_by_side(spline, lo, hi, times, values)
    g = [np.asarray(x, dtype=LD) for x in g]
    zero = np.zeros(g[0].shape, dtype=LD)
    gp = np.where(missing, LD(0), np.concatenate([g[0], g[1], zero, zero], axis=1))
    gv = np.where(missing, LD(0), np.concatenate([zero, zero, g[2], g[3]], axis=1))
    bars, tau_bar = vjp(spline, tau, gp, gv, np.zeros(tau.shape, dtype=LD))
    routed = lambda c: np.where(cls == c, tau_bar, LD(0))      # noqa: E731
    fold = lambda x: x.reshape(len(x), 4, k).sum(axis=1)      # noqa: E731
    end = routed(END).sum(axis=1)
    bars = list(bars)
    bars[6] = bars[6] + end + routed(KNOT).sum(axis=1)
    bars[7] = bars[7] + end
    return bars, fold(routed(LO)), fold(routed(HI))


def derivative_jvp_ld(spline, lo, hi, times, values, spline_dot, lo_dot, hi_dot, jvp=tr.jvp_ld):
    """Forward mode in longdouble (jvp=trajectory_ref.jvp_f64: with the evaluator's float64 restatement): the four value tangents (n, k), NaN where the value is.  One evaluator JVP at the same times with
    tau_dot = lo_dot (LO), hi_dot (HI), duration0_dot + duration1_dot (END), duration0_dot (KNOT), 0 (interior)."""
    k, tau, missing, cls = _side_by_side(spline, lo, hi, times, values)
    four = lambda x: np.tile(np.asarray(x, dtype=LD), (1, 4))      # noqa: E731
    d0_dot, d1_dot = (np.asarray(spline_dot[f], dtype=LD)[:, None] + np.zeros(tau.shape, dtype=LD) for f in (6, 7))
    tau_dot = np.select([cls == LO, cls == HI, cls == END, cls == KNOT], [four(lo_dot), four(hi_dot), d0_dot + d1_dot, d0_dot], LD(0))
    pd, vd, _ = jvp(spline, tau, spline_dot, tau_dot)
    pd, vd = np.where(missing, LD(np.nan), pd), np.where(missing, LD(np.nan), vd)
    return [pd[:, :k], pd[:, k:2 * k], vd[:, 2 * k:3 * k], vd[:, 3 * k:]]


# ---------------------------------------------------------------- inputs
def windows(spline, k, seed):
    """(lo, hi), (n, k) each: column 0 the whole spline, (-inf, +inf); column 1 (0, duration0) exactly; the others the sorted pair of two
    U(-0.1, 1.1) T draws -- both below 0 or both above T about once in a hundred: the NaN rule."""
    rng = np.random.default_rng(seed)
    d0, d1 = np.asarray(spline[6], dtype=np.float64), np.asarray(spline[7], dtype=np.float64)
    draws = np.sort(rng.uniform(-0.1, 1.1, (len(d0), k, 2)), axis=2) * (d0 + d1)[:, None, None]
    lo, hi = np.ascontiguousarray(draws[:, :, 0]), np.ascontiguousarray(draws[:, :, 1])
    lo[:, 0], hi[:, 0] = -np.inf, np.inf
    if k > 1:
        lo[:, 1], hi[:, 1] = 0.0, d0
    return lo, hi


def solved_golden(n):
    """The first n problems of tests/golden/f3_batch.npz as the gated solve left them: rest to rest, a ninth of them non-monotone with a
    knot velocity of rounding size."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f3_batch.npz"))
    pos, sol = z["pos"][:n], z["gated"][:n, :3]
    zero = np.zeros(len(pos))
    return [pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), zero, zero.copy(), sol[:, 0].copy(), sol[:, 1].copy(), sol[:, 2].copy()]


def knot_cases():
    """(spline of eight problems, lo (8, 1), hi (8, 1), which output sits on the knot): vel1 = 0 exactly and pos1 outside [pos0, pos2], above
    and below.  Cases 0-3: pos is extreme at the knot over the whole spline -- the velocity changes sign there, and its root sits on s = h
    of segment 0 and s = 0 of segment 1, not strictly inside.  Cases 4-7: acc changes sign across the knot, so vel has a kink extreme
    there (vel keeps its sign, pos goes on past pos1), over a window around the knot that stops before vel comes back.  All numbers are
    dyadic or small integers: the constants and the roots are exact in float64."""
    rows = [
        # pos0, pos1, pos2, vel0, vel2, duration0, duration1, lo, hi
        (0.0, 100.0, 0.0, 0.0, 0.0, 1.0, 1.0, -np.inf, np.inf, "pos_max"),
        (0.0, -100.0, 0.0, 0.0, 0.0, 2.0, 2.0, -np.inf, np.inf, "pos_min"),
        (0.0, 4.0, 1.0, 1.0, -1.0, 2.0, 1.0, -np.inf, np.inf, "pos_max"),
        (0.0, -4.0, -1.0, -1.0, 1.0, 2.0, 1.0, -np.inf, np.inf, "pos_min"),
        (0.0, -1.0, 0.0, 0.0, 5.0, 1.0, 1.0, 0.75, 1.25, "vel_max"),
        (0.0, 1.0, 0.0, 0.0, -5.0, 1.0, 1.0, 0.75, 1.25, "vel_min"),
        (0.0, -1.0, 0.5, 0.0, 16.0, 2.0, 0.5, 1.5, 2.125, "vel_max"),
        (0.0, 1.0, -0.5, 0.0, -16.0, 2.0, 0.5, 1.5, 2.125, "vel_min"),
    ]
    col = lambda j: np.array([r[j] for r in rows], dtype=np.float64)      # noqa: E731
    spline = [col(0), col(1), col(2), col(3), col(4), np.zeros(len(rows)), col(5), col(6)]
    return spline, col(7)[:, None].copy(), col(8)[:, None].copy(), [r[9] for r in rows]
