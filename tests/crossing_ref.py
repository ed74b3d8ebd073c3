"""Test-side restatements of the crossing times (rp_trajectory_crossing, csrc/trajectory.hip), on top of
tests/trajectory_ref.py: a spline is its list of eight arrays, a level an (n, k) array of positions.

    pieces_ld        the six monotone pieces of every problem in longdouble: the seven piece ends in time and pos there
    crossing_ld      the definition in longdouble: the first piece whose end positions hold the level, then 120 bisections
    derivative_ld / derivative_jvp_ld
                     the implicit-function derivative of the crossing time on top of trajectory_ref.vjp_ld / jvp_ld
    difference_is_a_yardstick
                     the queries at which a central difference with the tests' step is itself good to a tenth of their bound
    crossing_f64     the kernel's own rule in float64 (secant start, Newton steps kept in the bracket, the same stopping rule and trip
                     bound), with the trips each query takes: what the kernel cannot report.  1 / x is numpy's division where the
                     kernel has its refined reciprocal, so it is a restatement of the rule, not of the bits
    levels           queries for which the answer's existence is not a rounding question
"""
import numpy as np

import trajectory_ref as tr

LD = np.longdouble
TRIPS = 64                                  # kCrossTrips
TOL = 2.0 * np.finfo(np.float64).eps        # kCrossTol


def _breaks(va, acc0, jrk0, h, T):
    """The padded breakpoints 0 <= c1 <= c2 <= h of one segment (arrays, any shape), in the float type T."""
    with np.errstate(all="ignore"):
        a, b, c = jrk0 * T(0.5), acc0, va
        disc = b * b - T(4) * (a * c)
        ok = disc >= 0
        q = T(-0.5) * (b + np.copysign(np.sqrt(np.where(ok, disc, T(0))), b))
        r0 = np.where(ok & (a != 0), q / np.where(a != 0, a, T(1)), T(np.nan))
        r1 = np.where(ok, c / q, T(np.nan))
        in0, in1 = (r0 > 0) & (r0 < h), (r1 > 0) & (r1 < h)
        both, one = in0 & in1, in0 ^ in1
        r, other = np.where(in0, r0, r1), np.where(in0, r1, r0)
        larger = one & (other <= 0)             # the root inside is the larger one: the smaller is missing
        c1 = np.where(both, np.minimum(r0, r1), np.where(one & ~larger, r, T(0) * h))
        c2 = np.where(both, np.maximum(r0, r1), np.where(larger, r, h))
    return c1, c2


def _segments(spline, T, true_division):
    """Per segment (x0, va, acc0, jrk0, h) as (n, 1) columns of type T, and duration0; NaN durations by trajectory_ref's rule."""
    p0, p1, p2, v0, v2, v1, d0, d1 = tr._columns(spline, T)
    out = []
    with np.errstate(all="ignore"):
        for x0, x1, va, vb, h in ((p0, p1, v0, v1, d0), (p1, p2, v1, v2, d1)):
            if true_division:
                acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
                jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
            else:
                acc0, jrk0 = tr._constants_f64(x0, x1, va, vb, 1.0 / h)
            out.append((x0 + 0 * h, va + 0 * h, acc0, jrk0, h))
    return out, d0


def _pos(seg, s, T):
    x0, va, acc0, jrk0, _ = seg
    if T is LD:
        return x0 + (va + (acc0 + jrk0 * s / 3) * s / 2) * s
    return x0 + (va + (acc0 + jrk0 * (s * (1.0 / 3.0))) * (s * 0.5)) * s


def _vel(seg, s):
    _, va, acc0, jrk0, _ = seg
    return va + (acc0 + jrk0 * (s * 0.5)) * s


def _pieces(spline, T):
    """(segments, duration0, local piece ends (n, 2, 4), pos at the seven piece ends (n, 7)).  The knot's position is pos1 itself, as the
    evaluator gives it at tau = duration0."""
    segs, d0 = _segments(spline, T, T is LD)
    local, ends = [], []
    with np.errstate(all="ignore"):
        for g, seg in enumerate(segs):
            c1, c2 = _breaks(seg[1], seg[2], seg[3], seg[4], T)
            local.append(np.concatenate([0 * seg[4], c1, c2, seg[4]], axis=1))
            ends += [_pos(seg, 0 * seg[4], T), _pos(seg, c1, T), _pos(seg, c2, T)]
        ends.append(_pos(segs[1], segs[1][4], T))
    return segs, d0, np.stack(local, axis=1), np.concatenate(ends, axis=1)


def pieces_ld(spline):
    """(times (n, 7), positions (n, 7)) of the piece ends in longdouble, in time order."""
    _, d0, local, ends = _pieces(spline, LD)
    return np.concatenate([local[:, 0, :3], d0 + local[:, 1, :]], axis=1), ends


def _choose(ends, level):
    """Per query the first piece (0..5, -1: none) whose end positions hold the level, and the two end positions."""
    n, k = level.shape
    m = np.full((n, k), -1)
    p_lo, p_hi = np.zeros((n, k), dtype=ends.dtype), np.zeros((n, k), dtype=ends.dtype)
    with np.errstate(all="ignore"):
        for j in range(5, -1, -1):
            a, b = ends[:, j:j + 1], ends[:, j + 1:j + 2]
            holds = ((a <= level) & (level <= b)) | ((b <= level) & (level <= a))
            m = np.where(holds, j, m)
            p_lo, p_hi = np.where(holds, a, p_lo), np.where(holds, b, p_hi)
    return m, p_lo, p_hi


def _bracket(segs, local, m, T):
    """Per query: its segment's constants and the local ends (lo, hi) of its piece (piece -1: piece 0's, never used)."""
    seg = m >= 3
    j = np.where(m < 0, 0, m - 3 * seg)
    lo = np.where(seg, np.take_along_axis(local[:, 1, :], j, axis=1), np.take_along_axis(local[:, 0, :], j, axis=1))
    hi = np.where(seg, np.take_along_axis(local[:, 1, :], j + 1, axis=1), np.take_along_axis(local[:, 0, :], j + 1, axis=1))
    consts = tuple(np.where(seg, b, a) + T(0) * lo for a, b in zip(segs[0], segs[1]))
    return seg, consts, lo, hi


def crossing_ld(spline, level):
    """(time (n, k) longdouble with NaN where the level is not reached, piece (n, k) with -1 there, (lo, hi) the chosen piece in time)."""
    level = np.asarray(level, dtype=LD)
    segs, d0, local, ends = _pieces(spline, LD)
    m, p_lo, _ = _choose(ends, level)
    seg, consts, lo, hi = _bracket(segs, local, m, LD)
    offset = np.where(seg, d0, LD(0))
    piece = (offset + lo, offset + hi)
    with np.errstate(all="ignore"):
        g_lo = p_lo - level
        up = g_lo < 0
        a, b = lo.copy(), hi.copy()
        for _ in range(120):
            mid = a + (b - a) / 2
            g = _pos(consts, mid, LD) - level
            left = (g < 0) == up
            a, b = np.where(left, mid, a), np.where(left, b, mid)
        s = np.where(g_lo == 0, lo, a + (b - a) / 2)
        time = np.where(m < 0, LD(np.nan), offset + s)
    return time, m, piece


def derivative_ld(spline, time, g):
    """Reverse mode in longdouble at the times given (NaN: not reached): (eight spline gradients, level_bar) for the upstream g on time.
    w = g / vel, 0 where the time is NaN; level_bar = w; the spline's gradients are the evaluator's for g_pos = -w."""
    time = np.asarray(time, dtype=LD)
    missing = np.isnan(time)
    tau = np.where(missing, LD(0), time)
    with np.errstate(all="ignore"):
        vel = tr.forward_ld(spline, tau)[1]
        w = np.where(missing, LD(0), np.asarray(g, dtype=LD) / vel)
        zero = np.zeros(tau.shape, dtype=LD)
        bars, _ = tr.vjp_ld(spline, tau, -w, zero, zero)
    return bars, w


def derivative_jvp_ld(spline, time, spline_dot, level_dot):
    """Forward mode in longdouble: time_dot = (level_dot - pos_dot at fixed time) / vel, NaN where the time is."""
    time = np.asarray(time, dtype=LD)
    missing = np.isnan(time)
    tau = np.where(missing, LD(0), time)
    with np.errstate(all="ignore"):
        vel = tr.forward_ld(spline, tau)[1]
        pos_dot = tr.jvp_ld(spline, tau, spline_dot, np.zeros(tau.shape, dtype=LD))[0]
        return np.where(missing, LD(np.nan), (np.asarray(level_dot, dtype=LD) - pos_dot) / vel)


def difference_steps(spline, level):
    """The steps of the central differences, as the evaluator's tests take them: 1e-6 max(|x|, 1) per input, (eight arrays of n, (n, k))."""
    return [1e-6 * np.maximum(np.abs(np.asarray(a, dtype=np.float64)), 1.0) for a in spline], 1e-6 * np.maximum(np.abs(level), 1.0)


def difference_is_a_yardstick(spline, time, level):
    """Where a central difference of the crossing time with difference_steps is itself good to a tenth of the 1e-6 it is compared
    within, (n, k) bool.  The time's derivatives are (d level - d pos) / vel: one over the crossing velocity.  A step h in an input
    moves the crossing by dt = |d pos / d input| h / |vel| and the velocity there by dv = |d vel / d input| h + |acc| dt + |jrk| dt^2; the
    difference quotient of 1 / vel is off by about (dv / vel)^2 of itself (the next term of its expansion: for the level, f = 1 / vel(p)
    has f(3) h^2 / (6 f) = (acc h / vel^2)^2 (1 / 2 - jrk vel / (6 acc^2)) ).  Asked: (dv / vel)^2 <= 1e-7 for every one of the nine
    steps.  A property of the spline, the level and the step alone -- longdouble, nothing of the code under test enters."""
    time = np.asarray(time, dtype=LD)
    missing = np.isnan(time)
    tau = np.where(missing, LD(0), time)
    steps, level_step = difference_steps(spline, level)
    n = len(steps[0])
    zero = np.zeros(tau.shape, dtype=LD)
    with np.errstate(all="ignore"):
        _, vel, acc = tr.forward_ld(spline, tau)
        jrk = tr.jvp_ld(spline, tau, [np.zeros(n)] * 8, np.ones(tau.shape))[2]      # d acc / d tau
        worst = np.zeros(tau.shape, dtype=LD)
        for f in range(9):
            if f < 8:
                dots = [np.zeros(n) for _ in range(8)]
                dots[f] = steps[f]
                pos_dot, vel_dot, _ = tr.jvp_ld(spline, tau, dots, zero)
            else:
                pos_dot, vel_dot = np.asarray(level_step, dtype=LD), zero
            dt = np.abs(pos_dot / vel)
            dv = np.abs(vel_dot) + np.abs(acc) * dt + np.abs(jrk) * dt**2
            worst = np.maximum(worst, (dv / vel)**2)
    return ~missing & (np.asarray(worst, dtype=np.float64) <= 1e-7)


def crossing_f64(spline, level):
    """(time, vel, trips), (n, k) each: the kernel's rule in float64, trips the evaluations of pos a query makes (0: no search)."""
    level = np.asarray(level, dtype=np.float64)
    F = np.float64
    segs, d0, local, ends = _pieces(spline, F)
    m, p_lo, p_hi = _choose(ends, level)
    seg, c, lo, hi = _bracket(segs, local, m, F)
    lo, hi = lo.copy(), hi.copy()
    with np.errstate(all="ignore"):
        g_lo, g_hi = p_lo - level, p_hi - level
        search = (m >= 0) & (g_lo != 0)
        up = g_lo < 0
        tol = TOL * hi
        width = hi - lo
        best = np.where(np.abs(g_hi) < np.abs(g_lo), hi, lo)
        best_g = np.fmin(np.abs(g_lo), np.abs(g_hi))
        s = lo + width * (g_lo * (1.0 / (g_lo - g_hi)))
        s = np.where((s > lo) & (s < hi), s, lo + 0.5 * width)
        dx_old, dx = width.copy(), width.copy()
        trips = np.zeros(level.shape, dtype=np.int64)
        live = search.copy()
        last = np.zeros(level.shape, dtype=bool)
        for _ in range(TRIPS):
            if not live.any():
                break
            trips += live
            g = _pos(c, s, F) - level
            v = _vel(c, s)
            better = live & (np.abs(g) < best_g)
            best_g, best = np.where(better, np.abs(g), best_g), np.where(better, s, best)
            live = live & ~(g == 0) & ~last
            left = (g < 0) == up
            lo, hi = np.where(live & left, s, lo), np.where(live & ~left, s, hi)
            width = hi - lo
            live = live & (width > tol)
            step = g * (1.0 / v)
            nxt = s - step
            newton = (nxt > lo) & (nxt < hi) & (2.0 * np.abs(step) <= np.abs(dx_old))
            nxt = np.where(newton, nxt, lo + 0.5 * width)
            last = live & newton & (np.abs(c[2] + c[3] * s) * (step * step) <= (2.0 * tol) * np.abs(v))
            dx_old, dx = np.where(live, dx, dx_old), np.where(live, nxt - s, dx)
            live = live & (np.abs(dx) > tol)
            s = np.where(live, nxt, s)
        s = np.where(search, best, lo)
        time = np.where(m < 0, np.nan, np.where(seg, d0 + s, s))
        vel = np.where(m < 0, np.nan, _vel(c, s))
    return time, vel, np.where(search, trips, 0)


def levels(spline, k, seed, with_reached=False):
    """(n, k) query levels: 85 % reached -- P_m + u (P_m+1 - P_m), u ~ U(0.01, 0.99), the piece m drawn among those whose range is at least
    1e-6 max(X, 1) (the widest one if there is none) -- and 15 % unreached, beyond the spline's extreme values by (0.01 + u) of its span,
    u ~ U(0, 1).  with_reached: also the mask of the reached ones and each one's fraction u of its piece."""
    rng = np.random.default_rng(seed)
    _, ends = pieces_ld(spline)
    ends = np.asarray(ends, dtype=np.float64)
    n = len(ends)
    scale = tr.scales(spline)[0]                                   # max(X, 1), (n, 1)
    ranges = np.abs(np.diff(ends, axis=1))                         # (n, 6)
    eligible = ranges >= 1e-6 * scale
    eligible[~eligible.any(axis=1), :] = False
    widest = np.argmax(ranges, axis=1)
    score = np.where(eligible[:, None, :], rng.uniform(size=(n, k, 6)), -1.0)
    piece = np.where(eligible.any(axis=1)[:, None], np.argmax(score, axis=2), widest[:, None])
    u = rng.uniform(0.01, 0.99, (n, k))
    a, b = np.take_along_axis(ends, piece, axis=1), np.take_along_axis(ends, piece + 1, axis=1)
    inside = a + u * (b - a)
    low, high = ends.min(axis=1, keepdims=True), ends.max(axis=1, keepdims=True)
    beyond = (0.01 + rng.uniform(size=(n, k))) * (high - low)
    outside = np.where(rng.uniform(size=(n, k)) < 0.5, low - beyond, high + beyond)
    reached = rng.uniform(size=(n, k)) >= 0.15
    out = np.ascontiguousarray(np.where(reached, inside, outside))
    return (out, reached, u) if with_reached else out


def rest_to_rest(n, seed):
    """Random splines with vel0 = vel2 = 0 exactly: a velocity root sits on s = 0 of segment 0, which is not inside (0, h)."""
    sp = tr.random_states(n, seed)
    sp[3] = np.zeros(n)
    sp[4] = np.zeros(n)
    return sp
