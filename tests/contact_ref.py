"""Test-side restatements of the first time two vehicles moving in d axes come within a distance (rp_trajectory_contact, csrc/trajectory.hip;
DESIGN.md section 25), on top of tests/separation_ref.py.  Vehicles and queries are separation_ref's; new is a level (n, k) in units of squared
distance.  f(t) = the sum over the axes of (pos_Ac(t) - pos_Bc(t - delay))^2; the output is the earliest time in the clamped window at which
f is at the level, NaN where it never is.

    subpieces_ld     the definition's breakpoints in longdouble: separation_ref.candidates_ld in time order, an invalid candidate repeating
                     the one before it; (times, values, ok)
    contact_ld       the definition: the first sub-piece whose end values hold the level, 120 bisections of f_ld - level on it; an end value
                     equal to the level is the answer itself; (time, sub-piece index or -1, (t_lo, t_hi))
    contact_f64      the kernel's rule in float64, operation for operation (1 / x is numpy's division where the kernel has its refined
                     reciprocal): (time, rate, trips per query, the trips of its longest single search)
    rate_ld          f' in longdouble at given times
    derivative_ld / derivative_jvp_ld
                     the documented routing on trajectory_ref.vjp_ld / jvp_ld of each spline at the returned times
    difference_is_a_yardstick
                     meeting_ref's mask with f' in place of the closing velocity
    levels, family   the test inputs
"""
import numpy as np

import separation_ref as sr
import trajectory_ref as tr

LD = np.longdouble
EPS = 2.2e-16


def tmax(a, b, delay):
    """The largest of T_Ac and |delay| + T_Bc over the axes, (n, k)."""
    delay = np.asarray(delay, dtype=np.float64)
    most = np.zeros(delay.shape)
    for x, y in zip(a, b):
        most = np.maximum(most, np.maximum((x[6] + x[7])[:, None], np.abs(delay) + (y[6] + y[7])[:, None]))
    return most


def queries(a, level, lo, hi, delay):
    """(level, lo, hi, delay) as float64 (n, k) arrays; a level of (k,) is every problem's."""
    level = np.asarray(level, dtype=np.float64)
    k = level.shape[-1]
    lo, hi, delay = sr._queries(a, lo, hi, delay, k)
    return np.ascontiguousarray(np.broadcast_to(level, lo.shape)), lo, hi, delay


def subpieces_ld(a, b, lo=None, hi=None, delay=None, candidates=None):
    """(times, values, ok): the breakpoints in time order, lists of (n, k) longdouble arrays."""
    times, valid, values = candidates if candidates is not None else sr.candidates_ld(a, b, lo, hi, delay)
    bt, bv = [times[0]], [values[0]]
    for t, on, v in zip(times[1:], valid[1:], values[1:]):
        bt.append(np.where(on, t, bt[-1]))
        bv.append(np.where(on, v, bv[-1]))
    return bt, bv, valid[0]


def _choose(bt, bv, ok, level):
    m = np.full(level.shape, -1)
    zero = np.zeros(level.shape, dtype=bt[0].dtype)
    t_lo, t_hi, v_lo, v_hi = zero, zero, zero, zero
    with np.errstate(all="ignore"):
        for j in range(len(bt) - 2, -1, -1):
            p, q = bv[j], bv[j + 1]
            holds = ok & (((p <= level) & (level <= q)) | ((q <= level) & (level <= p)))
            m = np.where(holds, j, m)
            t_lo, t_hi, v_lo, v_hi = (np.where(holds, x, y) for x, y in ((bt[j], t_lo), (bt[j + 1], t_hi), (p, v_lo), (q, v_hi)))
    return m, t_lo, t_hi, v_lo, v_hi


def contact_ld(a, b, level, lo=None, hi=None, delay=None, subpieces=None):
    """(time (n, k) longdouble, NaN where the level is not reached; sub-piece (n, k), -1 there; (t_lo, t_hi) of the sub-piece).  The level
    may be longdouble."""
    _, lo, hi, delay = queries(a, np.asarray(level, dtype=np.float64), lo, hi, delay)
    level = np.broadcast_to(np.asarray(level, dtype=LD), lo.shape)
    bt, bv, ok = subpieces if subpieces is not None else subpieces_ld(a, b, lo, hi, delay)
    m, t_lo, t_hi, v_lo, v_hi = _choose(bt, bv, ok & np.isfinite(level), level)
    with np.errstate(all="ignore"):
        up = (v_lo - level) < 0
        p, q = t_lo.copy(), t_hi.copy()
        for _ in range(120):
            mid = p + (q - p) / 2
            left = ((sr.f_ld(a, b, mid, delay)[0] - level) < 0) == up
            p, q = np.where(left, mid, p), np.where(left, q, mid)
        t = np.where(v_lo == level, t_lo, np.where(v_hi == level, t_hi, p + (q - p) / 2))
    return np.where(m < 0, LD(np.nan), t), m, (t_lo, t_hi)


def rate_ld(a, b, t, delay, forward=tr.forward_ld, T=LD):
    """f' = 2 times the sum of D_c D_c' at the times t (n, k)."""
    t = np.asarray(t, dtype=T)
    tb = t - np.asarray(delay, dtype=T)
    total = np.zeros(t.shape, dtype=T)
    for x, y in zip(a, b):
        fa, fb = forward(x, t), forward(y, tb)
        total = total + (fa[0] - fb[0]) * (fa[1] - fb[1])
    return 2 * total


def _quintic_f0(a, segs_a, segs_b, kA, kB, dl, c):
    """separation_ref._quintic with F0 = the sum of X_c^2 beside it, in the kernel's order of operations."""
    T = np.float64
    g, F0 = None, None
    for x in range(len(a)):
        seg_a, seg_b = kA[x] <= c, kB[x] <= c
        ca = [np.where(seg_a, segs_a[x][1][i], segs_a[x][0][i]) for i in range(4)]
        cb = [np.where(seg_b, segs_b[x][1][i], segs_b[x][0][i]) for i in range(4)]
        sa, sb = sr._cubic(ca, np.where(seg_a, c - kA[x], c), T), sr._cubic(cb, np.where(seg_b, c - kB[x], c - dl), T)
        X, V, A, J = (p - q for p, q in zip(sa, sb))
        p0, p1, p2, p3 = X, V, A * T(0.5), J * (T(1) / T(6))
        q0, q1, q2 = V, A, J * T(0.5)
        t = [p0 * q0, p0 * q1 + p1 * q0, (p0 * q2 + p1 * q1) + p2 * q0, (p1 * q2 + p2 * q1) + p3 * q0, p2 * q2 + p3 * q1, p3 * q2]
        g = [T(0) + v for v in t] if g is None else [u + v for u, v in zip(g, t)]
        F0 = T(0) + p0 * p0 if F0 is None else F0 + p0 * p0
    return g, F0


def contact_f64(a, b, level, lo=None, hi=None, delay=None):
    """(time, rate, trips, deepest) by the kernel's rule in float64: a query that is NaN by its inputs makes no search; the walk of a query
    ends with the piece that holds its answer and at a piece after the first that starts at b."""
    T = np.float64
    level, lo, hi, delay = queries(a, level, lo, hi, delay)
    wa, wb, ok, kA, kB, dl = sr._setup(a, b, lo, hi, delay, T)
    ok = ok & np.isfinite(level)
    segs_a, segs_b = [sr.gr._segments(x, T) for x in a], [sr.gr._segments(x, T) for x in b]
    value = lambda t, on: sr._value(a, b, t, dl, on, tr.forward_f64, T)[0]      # noqa: E731
    found, t_found = np.zeros(wa.shape, dtype=bool), np.full(wa.shape, np.nan)
    trips, deepest = np.zeros(wa.shape, dtype=np.int64), np.zeros(wa.shape, dtype=np.int64)
    nan = np.full(wa.shape, np.nan)
    with np.errstate(all="ignore"):
        c, f_c = wa.copy(), value(wa, ok)
        for piece in range(2 * len(a) + 1):
            live = ok & ~found & ((c < wb) | (piece == 0))
            if not live.any():
                break
            cl = np.where(live, c, nan)      # a query that has left the walk: NaN, no change of sign, no search
            e = sr._piece_end(cl, wb, kA, kB)
            g, F0 = _quintic_f0(a, segs_a, segs_b, kA, kB, dl, cl)
            length, tol = e - cl, sr.TOL * e
            g1 = [g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4], 5.0 * g[5]]
            g2 = [2.0 * g[2], 6.0 * g[3], 12.0 * g[4], 20.0 * g[5]]
            r3 = sr._velocity_breaks(6.0 * g[3], 24.0 * g[4], 120.0 * g[5], length)
            r2, n2, m2 = sr._roots_between(g2, list(r3), length, tol)
            r1, n1, m1 = sr._roots_between(g1, r2, length, tol)
            r0, n0, m0 = sr._roots_between(g, r1, length, tol)
            trips, deepest = trips + n2 + n1 + n0, np.maximum(np.maximum(deepest, m2), np.maximum(m1, m0))
            here = np.zeros(wa.shape, dtype=bool)
            t_lo, t_hi, f_lo, f_hi = nan, nan, nan, nan
            t_prev, f_prev = cl, f_c
            for j in range(6):
                if j < 5:
                    u = r0[j]
                    t = cl + u
                    real = live & (u > 0) & (u < length) & (wa < t) & (t < wb)
                else:
                    t, real = e, live
                f = value(t, real)
                t_next, f_next = np.where(real, t, t_prev), np.where(real, f, f_prev)
                holds = live & (((f_prev <= level) & (level <= f_next)) | ((f_next <= level) & (level <= f_prev)))
                first = holds & ~here
                t_lo, t_hi, f_lo, f_hi = (np.where(first, x, y) for x, y in ((t_prev, t_lo), (t_next, t_hi), (f_prev, f_lo), (f_next, f_hi)))
                here = here | holds
                t_prev, f_prev = t_next, f_next
            search = here & (f_lo != level)
            h = [F0 - level, g[0] * 2.0, g[1] * (2.0 / 2.0), g[2] * (2.0 / 3.0), g[3] * (2.0 / 4.0), g[4] * (2.0 / 5.0), g[5] * (2.0 / 6.0)]
            u, n = sr._search(h, t_lo - cl, t_hi - cl, f_lo - level, f_hi - level, tol, search)
            t = cl + u
            t = np.where(t < t_lo, t_lo, np.where(t > t_hi, t_hi, t))
            t_found = np.where(here, np.where(search, t, t_lo), t_found)
            found = found | here
            trips, deepest = trips + n, np.maximum(deepest, n)
            c, f_c = np.where(live, e, c), np.where(live, f_prev, f_c)
        at = np.where(found, t_found, 0.0)
        rate = _rate_f64(a, b, at, np.where(found, dl, 0.0))
    return np.where(found, t_found, np.nan), np.where(found, rate, np.nan), trips, deepest


def _rate_f64(a, b, t, dl):
    """2.0 times the sum in axis order from 0.0 of (pos_A - pos_B) (vel_A - vel_B) on the evaluator's float64 restatement."""
    total = np.zeros(t.shape)
    for x, y in zip(a, b):
        fa, fb = tr.forward_f64(x, t), tr.forward_f64(y, t - dl)
        total = total + (fa[0] - fb[0]) * (fa[1] - fb[1])
    return 2.0 * total


# ---------------------------------------------------------------- derivatives
def _at(time, delay, T=LD):
    time = np.asarray(time, dtype=T)
    missing = np.isnan(time)
    with np.errstate(all="ignore"):
        return missing, np.where(missing, T(0), time), np.where(missing, T(0), time - np.asarray(delay, dtype=T))


def _gaps(a, b, tau_a, tau_b, forward, T):
    """Per axis (D_c, D_c') and f' = 2 times the sum of their products."""
    per, total = [], np.zeros(tau_a.shape, dtype=T)
    for x, y in zip(a, b):
        fa, fb = forward(x, tau_a), forward(y, tau_b)
        per.append((fa[0] - fb[0], fa[1] - fb[1]))
        total = total + per[-1][0] * per[-1][1]
    return per, 2 * total


def derivative_ld(a, b, delay, time, g, vjp=tr.vjp_ld, forward=tr.forward_ld, T=LD):
    """Reverse mode at the times given (NaN: no contact): (A's d lists of eight gradients, B's, level_bar, delay_bar (n, k)) for the upstream
    g on the time.  w = g / rate, 0 where the time is NaN; level_bar = w; per axis A_c's gradients are the evaluator's at the time for
    g_pos = -2 w D_c, B_c's at time - delay for g_pos = +2 w D_c, and delay_bar is minus the sum of B's tau_bar."""
    missing, tau_a, tau_b = _at(time, delay, T)
    with np.errstate(all="ignore"):
        per, rate = _gaps(a, b, tau_a, tau_b, forward, T)
        w = np.where(missing, T(0), np.asarray(g, dtype=T) / rate)
        zero = np.zeros(tau_a.shape, dtype=T)
        bars_a, bars_b, delay_bar = [], [], zero
        for x, y, (gap, _) in zip(a, b, per):
            gp = 2 * w * np.where(missing, T(0), gap)
            bars_a.append(list(vjp(x, tau_a, -gp, zero, zero)[0]))
            bar_y, tau_bar = vjp(y, tau_b, gp, zero, zero)
            bars_b.append(list(bar_y))
            delay_bar = delay_bar - tau_bar
    return bars_a, bars_b, w, delay_bar


def derivative_jvp_ld(a, b, delay, time, a_dot, b_dot, level_dot, delay_dot, jvp=tr.jvp_ld, forward=tr.forward_ld, T=LD):
    """Forward mode: time_dot = (level_dot - the sum of 2 D_c (pos_Ac_dot - pos_Bc_dot)) / rate with B's tau_dot = -delay_dot, NaN where the
    time is."""
    missing, tau_a, tau_b = _at(time, delay, T)
    with np.errstate(all="ignore"):
        per, rate = _gaps(a, b, tau_a, tau_b, forward, T)
        total = np.asarray(level_dot, dtype=T) + np.zeros(tau_a.shape, dtype=T)
        for x, y, xd, yd, (gap, _) in zip(a, b, a_dot, b_dot, per):
            pa = jvp(x, tau_a, xd, np.zeros(tau_a.shape, dtype=T))[0]
            pb = jvp(y, tau_b, yd, -np.asarray(delay_dot, dtype=T))[0]
            total = total - 2 * gap * (pa - pb)
        return np.where(missing, T(np.nan), total / rate)


def difference_steps(a, b, level, delay):
    """The steps of the central differences: 1e-6 max(|x|, 1) per input -- (A's d lists of eight arrays of n, B's, the level's (n, k), the
    delay's)."""
    step = lambda x: 1e-6 * np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 1.0)      # noqa: E731
    return [[step(v) for v in x] for x in a], [[step(v) for v in y] for y in b], step(level), step(delay)


def difference_is_a_yardstick(a, b, level, delay, time):
    """meeting_ref.difference_is_a_yardstick with rate = f'(time) in place of the closing velocity: a step h in an input moves the contact by
    dt = |df / d input| h / |rate| and the rate there by dv = |df' / d input| h + |f''| dt + |f'''| dt^2; asked: (dv / rate)^2 <= 1e-7 for
    every one of the 16 d + 2 steps.  longdouble on the splines, the query and the step alone."""
    missing, tau_a, tau_b = _at(time, delay)
    steps_a, steps_b, level_step, delay_step = difference_steps(a, b, level, delay)
    n = len(steps_a[0][0])
    zero, one = np.zeros(tau_a.shape, dtype=LD), np.ones(tau_a.shape)
    none = [np.zeros(n)] * 8
    with np.errstate(all="ignore"):
        D, rate, f2, f3 = [], zero, zero, zero
        d_delay, dv_delay = zero, zero
        for x, y in zip(a, b):
            fa, fb = tr.forward_ld(x, tau_a), tr.forward_ld(y, tau_b)
            jrk = tr.jvp_ld(x, tau_a, none, one)[2] - tr.jvp_ld(y, tau_b, none, one)[2]
            gap, vel, acc = fa[0] - fb[0], fa[1] - fb[1], fa[2] - fb[2]
            D.append((gap, vel))
            rate = rate + 2 * gap * vel
            f2 = f2 + 2 * (vel * vel + gap * acc)
            f3 = f3 + 2 * (3 * vel * acc + gap * jrk)
            d_delay = d_delay + 2 * gap * fb[1]
            dv_delay = dv_delay + 2 * (fb[1] * vel + gap * fb[2])
        moves = [(np.asarray(level_step, dtype=LD), zero), (np.abs(d_delay) * delay_step, np.abs(dv_delay) * delay_step)]
        for x in range(len(a)):
            gap, vel = D[x]
            for spline, tau, steps in ((a[x], tau_a, steps_a[x]), (b[x], tau_b, steps_b[x])):
                for f in range(8):
                    dots = [np.zeros(n) for _ in range(8)]
                    dots[f] = steps[f]
                    pos_dot, vel_dot = tr.jvp_ld(spline, tau, dots, zero)[:2]
                    moves.append((2 * gap * pos_dot, 2 * (pos_dot * vel + gap * vel_dot)))
        worst = np.zeros(tau_a.shape, dtype=LD)
        for f_dot, rate_dot in moves:
            dt = np.abs(f_dot / rate)
            dv = np.abs(rate_dot) + np.abs(f2) * dt + np.abs(f3) * dt**2
            worst = np.maximum(worst, (dv / rate)**2)
    return ~missing & (np.asarray(worst, dtype=np.float64) <= 1e-7)


# ---------------------------------------------------------------- inputs
def levels(a, b, lo, hi, delay, seed, subpieces=None):
    """(level (n, k), reached (n, k) bool, the number of queries without an eligible sub-piece).  85 % reached -- f_m + u (f_m+1 - f_m),
    u ~ U(0.01, 0.99), the sub-piece m drawn among those of the longdouble definition whose range is at least 1e-6 of the largest f among
    the query's breakpoints (section 24's distance unit) -- and 15 % unreached, beyond the window's least or greatest f by (0.01 + u)
    max(span, 1), u ~ U(0, 1).  A query without an eligible sub-piece gets an unreached level and is counted (no window: the level 0)."""
    rng = np.random.default_rng(seed)
    _, bv, ok = subpieces if subpieces is not None else subpieces_ld(a, b, lo, hi, delay)
    with np.errstate(all="ignore"):
        ends = np.stack([np.asarray(np.where(ok & ~np.isnan(v), v, 0), dtype=np.float64) for v in bv], axis=2)
    n, k = ok.shape
    m = ends.shape[2] - 1
    ranges = np.abs(np.diff(ends, axis=2))
    eligible = (ranges >= 1e-6 * ends.max(axis=2)[:, :, None]) & (ranges > 0) & ok[:, :, None]
    some = eligible.any(axis=2)
    piece = np.argmax(np.where(eligible, rng.uniform(size=(n, k, m)), -1.0), axis=2)[:, :, None]
    u = rng.uniform(0.01, 0.99, (n, k))
    p, q = np.take_along_axis(ends, piece, axis=2)[:, :, 0], np.take_along_axis(ends, piece + 1, axis=2)[:, :, 0]
    inside = p + u * (q - p)
    low, high = ends.min(axis=2), ends.max(axis=2)
    beyond = (0.01 + rng.uniform(size=(n, k))) * np.maximum(high - low, 1.0)
    outside = np.where(rng.uniform(size=(n, k)) < 0.5, low - beyond, high + beyond)
    reached = (rng.uniform(size=(n, k)) >= 0.15) & some
    return np.ascontiguousarray(np.where(reached, inside, np.where(ok, outside, 0.0))), reached, int((~some).sum())


def family(name, n=512, k=8, d=2):
    """(A, B, level, lo, hi, delay, reached, the count of queries without an eligible sub-piece, the longdouble sub-pieces): section 24's
    family with levels of seed 100 + d."""
    a, b, lo, hi, delay = sr.family(name, n, k, d)
    sub = subpieces_ld(a, b, lo, hi, delay)
    level, reached, odd = levels(a, b, lo, hi, delay, 100 + d, sub)
    return a, b, level, lo, hi, delay, reached, odd, sub
