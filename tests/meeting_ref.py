"""Test-side restatements of the meeting times of two splines (rp_trajectory_meeting, csrc/trajectory.hip), on top of
tests/gap_ref.py, tests/crossing_ref.py, tests/tracking_ref.py and tests/trajectory_ref.py: a spline is its list of eight arrays, a query a
level, a window lo, hi and a delay, four (n, k) arrays (None: 0 / -inf / +inf / 0).  D(t) = pos_A(t) - pos_B(t - delay).

    subpieces_ld     the definition's ten breakpoints in longdouble, from gap_ref.candidates_ld: times and gap values in time order, each
                     sub-piece's piece start, and which queries have a window at all
    meeting_ld       the definition: the first sub-piece whose end values hold the level, then 120 bisections on trajectory_ref's
                     longdouble forward
    meeting_f64      the kernel's rule in float64 (the breakpoints through gap_ref's float64 candidates, the search of crossing_ref on the
                     piece's local cubic as tracking_ref forms it), with the trips each query takes.  1 / x is numpy's division where the
                     kernel has its refined reciprocal: a restatement of the rule, not of the bits
    derivative_ld / derivative_jvp_ld
                     the implicit-function derivative on trajectory_ref.vjp_ld / jvp_ld of each spline
    difference_is_a_yardstick
                     the queries at which a central difference with the tests' step is itself good to a tenth of their bound
    levels           queries whose answer's existence is not a rounding question
    family, hand_made
                     the test inputs
"""
import numpy as np

import crossing_ref as cr
import gap_ref as gr
import tracking_ref as kr
import trajectory_ref as tr

LD = np.longdouble
EPS = 2.2e-16
KNOTS = (3, 6)      # the breakpoints that end pieces 0 and 1


def tmax(a, b, delay):
    """max(T_A, |delay| + T_B), (n, k)."""
    return np.maximum((a[6] + a[7])[:, None], np.abs(delay) + (b[6] + b[7])[:, None])


def queries(a, level, lo, hi, delay):
    """(level, lo, hi, delay) as float64 (n, k) arrays: None is 0 / -inf / +inf / 0, all None one whole-domain query per problem."""
    k = next((np.shape(x)[1] for x in (level, lo, hi, delay) if x is not None), 1)
    lo, hi, delay = gr._queries(a, lo, hi, delay, k)
    return (np.zeros(lo.shape) if level is None else np.asarray(level, dtype=np.float64)), lo, hi, delay


def _subpieces(a, b, lo, hi, delay, T):
    """(times, values: ten (n, k) arrays of type T in time order; starts: the piece start c of each of the nine sub-pieces; ok).  A root
    that is no candidate repeats the breakpoint before it; a knot outside [a, b] is the end it is clamped to."""
    times, valid, values = gr._candidates(a, b, lo, hi, delay, T)
    ok, wa, wb = valid[0], times[0], times[9]
    bt, bv, starts, c = [wa], [values[0]], [], wa
    with np.errstate(all="ignore"):
        for i in range(1, 10):
            if i in KNOTS:
                before = times[i] < wa
                t = np.where(valid[i], times[i], np.where(before, wa, wb))
                v = np.where(valid[i], values[i], np.where(before, values[0], values[9]))
            elif i == 9:
                t, v = wb, values[9]
            else:
                t, v = np.where(valid[i], times[i], bt[-1]), np.where(valid[i], values[i], bv[-1])
            starts.append(c)
            bt.append(t)
            bv.append(v)
            if i in KNOTS:
                c = t
    return bt, bv, starts, ok


def subpieces_ld(a, b, lo=None, hi=None, delay=None):
    return _subpieces(a, b, lo, hi, delay, LD)


def _choose(bt, bv, starts, ok, level):
    """Per query the first sub-piece (0..8, -1: none) whose end values hold the level, its ends in time, their values, its piece start."""
    m = np.full(level.shape, -1)
    zero = np.zeros(level.shape, dtype=bt[0].dtype)
    t_lo, t_hi, v_lo, v_hi, c = zero, zero, zero, zero, zero
    with np.errstate(all="ignore"):
        for j in range(8, -1, -1):
            p, q = bv[j], bv[j + 1]
            holds = ok & (((p <= level) & (level <= q)) | ((q <= level) & (level <= p)))
            m = np.where(holds, j, m)
            t_lo, t_hi, v_lo, v_hi, c = (np.where(holds, x, y) for x, y in ((bt[j], t_lo), (bt[j + 1], t_hi), (p, v_lo), (q, v_hi), (starts[j], c)))
    return m, t_lo, t_hi, v_lo, v_hi, c


def gap_ld(a, b, t, delay):
    """D and D' in longdouble at the times t (n, k)."""
    fa, fb = tr.forward_ld(a, t), tr.forward_ld(b, t - np.asarray(delay, dtype=LD))
    return fa[0] - fb[0], fa[1] - fb[1]


def meeting_ld(a, b, level=None, lo=None, hi=None, delay=None):
    """(time (n, k) longdouble with NaN where the level is not reached, sub-piece (n, k) with -1 there, (lo, hi) the chosen sub-piece in
    time).  The level may be longdouble."""
    _, lo, hi, delay = queries(a, level if level is None else np.asarray(level, dtype=np.float64), lo, hi, delay)
    level = np.zeros(lo.shape, dtype=LD) if level is None else np.asarray(level, dtype=LD)
    m, t_lo, t_hi, v_lo, v_hi, _ = _choose(*subpieces_ld(a, b, lo, hi, delay), level)
    with np.errstate(all="ignore"):
        g_lo = v_lo - level
        up = g_lo < 0
        p, q = t_lo.copy(), t_hi.copy()
        for _ in range(120):
            mid = p + (q - p) / 2
            left = ((gap_ld(a, b, mid, delay)[0] - level) < 0) == up
            p, q = np.where(left, mid, p), np.where(left, q, mid)
        # on a monotone sub-piece an end value equal to the level is the answer itself (the bisection would stop short of a touch)
        t = np.where(g_lo == 0, t_lo, np.where(v_hi == level, t_hi, p + (q - p) / 2))
    return np.where(m < 0, LD(np.nan), t), m, (t_lo, t_hi)


def _search_f64(X, V, A, J, level, lo, hi, g_lo, g_hi, tol, search):
    """bracket_search of csrc/trajectory.hip in float64, as crossing_ref.crossing_f64 restates it: (the point of smallest |g|, trips)."""
    c = (X, V, A, J, None)
    lo, hi = lo.copy(), hi.copy()
    with np.errstate(all="ignore"):
        up = g_lo < 0
        width = hi - lo
        best = np.where(np.abs(g_hi) < np.abs(g_lo), hi, lo)
        best_g = np.fmin(np.abs(g_lo), np.abs(g_hi))
        s = lo + width * (g_lo * (1.0 / (g_lo - g_hi)))
        s = np.where((s > lo) & (s < hi), s, lo + 0.5 * width)
        dx_old, dx = width.copy(), width.copy()
        trips = np.zeros(level.shape, dtype=np.int64)
        live = search.copy()
        last = np.zeros(level.shape, dtype=bool)
        for _ in range(cr.TRIPS):
            if not live.any():
                break
            trips += live
            g = cr._pos(c, s, np.float64) - level
            v = cr._vel(c, s)
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
            last = live & newton & (np.abs(A + J * s) * (step * step) <= (2.0 * tol) * np.abs(v))
            dx_old, dx = np.where(live, dx, dx_old), np.where(live, nxt - s, dx)
            live = live & (np.abs(dx) > tol)
            s = np.where(live, nxt, s)
    return best, trips


def meeting_f64(a, b, level=None, lo=None, hi=None, delay=None):
    """(time, relvel, trips), (n, k) each: the kernel's rule in float64, trips the evaluations of the local cubic a query makes (0: no
    search)."""
    F = np.float64
    level, lo, hi, delay = queries(a, level, lo, hi, delay)
    m, t_lo, t_hi, v_lo, v_hi, c = _choose(*_subpieces(a, b, lo, hi, delay, F), level)
    _, _, kA, kB, _, _ = gr._domain(a, b, delay)
    with np.errstate(all="ignore"):
        g_lo, g_hi = v_lo - level, v_hi - level
        search = (m >= 0) & (g_lo != 0)
        seg_a, seg_b = kA <= c, kB <= c
        XA, VA, AA, JA = kr._local(kr._constants(a, F), seg_a, np.where(seg_a, c - kA, c), F)
        XB, VB, AB, JB = kr._local(kr._constants(b, F), seg_b, np.where(seg_b, c - kB, c - delay), F)
        u, trips = _search_f64(XA - XB, VA - VB, AA - AB, JA - JB, level, t_lo - c, t_hi - c, g_lo, g_hi, cr.TOL * t_hi, search)
        t = c + u
        t = np.where(t < t_lo, t_lo, np.where(t > t_hi, t_hi, t))      # kept inside the sub-piece
        t = np.where(search, t, t_lo)
        at = np.where(m < 0, 0.0, t)
        relvel = tr.forward_f64(a, at)[1] - tr.forward_f64(b, at - np.where(m < 0, 0.0, delay))[1]
    return np.where(m < 0, np.nan, t), np.where(m < 0, np.nan, relvel), np.where(search, trips, 0)


# ---------------------------------------------------------------- derivatives
def _at(time, delay, T=LD):
    """(where there is no meeting; A's times and B's, those minus the delay, 0 there)"""
    time = np.asarray(time, dtype=T)
    missing = np.isnan(time)
    with np.errstate(all="ignore"):
        return missing, np.where(missing, T(0), time), np.where(missing, T(0), time - np.asarray(delay, dtype=T))


def derivative_ld(a, b, delay, time, g, vjp=tr.vjp_ld, forward=tr.forward_ld, T=LD):
    """Reverse mode at the times given (NaN: no meeting): (A's eight gradients, B's eight, level_bar, delay_bar (n, k)) for the upstream g
    on the time.  w = g / relvel, 0 where the time is NaN; level_bar = w; A's gradients are the evaluator's at the time for g_pos = -w,
    B's at time - delay for g_pos = +w, and delay_bar is minus B's tau_bar.  vjp, forward, T: trajectory_ref's float64 restatements in
    place of its longdouble ones."""
    missing, tau_a, tau_b = _at(time, delay, T)
    with np.errstate(all="ignore"):
        relvel = forward(a, tau_a)[1] - forward(b, tau_b)[1]
        w = np.where(missing, T(0), np.asarray(g, dtype=T) / relvel)
        zero = np.zeros(tau_a.shape, dtype=T)
        bars_a, _ = vjp(a, tau_a, -w, zero, zero)
        bars_b, tau_bar = vjp(b, tau_b, w, zero, zero)
    return list(bars_a), list(bars_b), w, -tau_bar


def derivative_jvp_ld(a, b, delay, time, a_dot, b_dot, level_dot, delay_dot, jvp=tr.jvp_ld, forward=tr.forward_ld, T=LD):
    """Forward mode: time_dot = (level_dot - pos_A_dot + pos_B_dot) / relvel with B's tau_dot = -delay_dot, NaN where the time is."""
    missing, tau_a, tau_b = _at(time, delay, T)
    with np.errstate(all="ignore"):
        relvel = forward(a, tau_a)[1] - forward(b, tau_b)[1]
        pa = jvp(a, tau_a, a_dot, np.zeros(tau_a.shape, dtype=T))[0]
        pb = jvp(b, tau_b, b_dot, -np.asarray(delay_dot, dtype=T))[0]
        return np.where(missing, T(np.nan), (np.asarray(level_dot, dtype=T) - pa + pb) / relvel)


def difference_steps(a, b, level, delay):
    """The steps of the central differences: 1e-6 max(|x|, 1) per input -- (A's eight arrays of n, B's eight, the level's (n, k), the
    delay's)."""
    step = lambda x: 1e-6 * np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 1.0)      # noqa: E731
    return [step(x) for x in a], [step(x) for x in b], step(level), step(delay)


def difference_is_a_yardstick(a, b, level, delay, time):
    """Where a central difference of the meeting time with difference_steps is itself good to a tenth of the 1e-6 it is compared within,
    (n, k) bool: crossing_ref.difference_is_a_yardstick for two splines.  Every derivative of the time is something over the closing
    velocity relvel = D'(time).  A step h in an input moves the meeting by dt = |d D / d input| h / |relvel| and the closing velocity there
    by dv = |d D' / d input| h + |D''| dt + |D'''| dt^2; the difference quotient of 1 / relvel is off by about (dv / relvel)^2 of itself.
    Asked: (dv / relvel)^2 <= 1e-7 for every one of the eighteen steps (sixteen spline inputs, the level, the delay: d D / d delay =
    vel_B, d D' / d delay = acc_B).  A property of the splines, the query and the step alone -- longdouble, nothing of the code under test
    enters."""
    missing, tau_a, tau_b = _at(time, delay)
    steps_a, steps_b, level_step, delay_step = difference_steps(a, b, level, delay)
    n = len(steps_a[0])
    zero, one = np.zeros(tau_a.shape, dtype=LD), np.ones(tau_a.shape)
    none = [np.zeros(n)] * 8
    with np.errstate(all="ignore"):
        fa, fb = tr.forward_ld(a, tau_a), tr.forward_ld(b, tau_b)
        relvel, relacc = fa[1] - fb[1], fa[2] - fb[2]
        reljrk = tr.jvp_ld(a, tau_a, none, one)[2] - tr.jvp_ld(b, tau_b, none, one)[2]      # d acc / d tau of each
        moves = [(np.asarray(level_step, dtype=LD), zero), (np.abs(fb[1]) * delay_step, np.abs(fb[2]) * delay_step)]
        for spline, tau, steps in ((a, tau_a, steps_a), (b, tau_b, steps_b)):
            for f in range(8):
                dots = [np.zeros(n) for _ in range(8)]
                dots[f] = steps[f]
                moves.append(tr.jvp_ld(spline, tau, dots, zero)[:2])
        worst = np.zeros(tau_a.shape, dtype=LD)
        for pos_dot, vel_dot in moves:
            dt = np.abs(pos_dot / relvel)
            dv = np.abs(vel_dot) + np.abs(relacc) * dt + np.abs(reljrk) * dt**2
            worst = np.maximum(worst, (dv / relvel)**2)
    return ~missing & (np.asarray(worst, dtype=np.float64) <= 1e-7)


# ---------------------------------------------------------------- inputs
def levels(a, b, lo, hi, delay, seed):
    """(level (n, k), reached (n, k) bool, the number of queries without an eligible sub-piece).  85 % reached -- D_m + u (D_m+1 - D_m),
    u ~ U(0.01, 0.99), the sub-piece m drawn among those of the longdouble definition whose range is at least 1e-6 of the scale -- and 15 %
    unreached, beyond the windowed extreme gaps by (0.01 + u) of their span, u ~ U(0, 1).  A query without an eligible sub-piece (no
    window: the level 0; a gap that does not move: beyond it by (0.01 + u) of the scale) is unreached and counted."""
    rng = np.random.default_rng(seed)
    _, bv, _, ok = subpieces_ld(a, b, lo, hi, delay)
    ends = np.stack([np.asarray(np.where(ok, v, 0), dtype=np.float64) for v in bv], axis=2)      # (n, k, 10)
    n, k = ok.shape
    sc = gr.scale(a, b)[:, :, None]
    ranges = np.abs(np.diff(ends, axis=2))
    eligible = (ranges >= 1e-6 * sc) & ok[:, :, None]
    some = eligible.any(axis=2)
    piece = np.argmax(np.where(eligible, rng.uniform(size=(n, k, 9)), -1.0), axis=2)[:, :, None]
    u = rng.uniform(0.01, 0.99, (n, k))
    p, q = np.take_along_axis(ends, piece, axis=2)[:, :, 0], np.take_along_axis(ends, piece + 1, axis=2)[:, :, 0]
    inside = p + u * (q - p)
    low, high = ends.min(axis=2), ends.max(axis=2)
    beyond = (0.01 + rng.uniform(size=(n, k))) * np.where(some, high - low, sc[:, :, 0])
    outside = np.where(rng.uniform(size=(n, k)) < 0.5, low - beyond, high + beyond)
    reached = (rng.uniform(size=(n, k)) >= 0.15) & some
    return np.ascontiguousarray(np.where(reached, inside, np.where(ok, outside, 0.0))), reached, int((~some).sum())


def family(name, n=512, k=8):
    """(A, B, level, lo, hi, delay, reached, the count of queries without an eligible sub-piece): section 18's families -- `random`
    unsolved pairs, `solved` pairs of tests/golden/f3_batch.npz, the delayed `follower` -- with its delays and windows."""
    if name == "random":
        a, b = gr.random_pair(n)
        delay = gr.delays(a, b, k, 41)
    else:
        a, b = gr.solved_pair(n)
        if name == "follower":
            b = gr.follower(a)
        delay = gr.delays(a, b, k, 43 if name == "follower" else 42, follow=name == "follower")
    lo, hi = gr.windows(a, b, delay, 44)
    level, reached, odd = levels(a, b, lo, hi, delay, 45)
    return a, b, level, lo, hi, delay, reached, odd


def standing(a):
    """A vehicle that stands still at 0 for as long as `a` drives: with it, a delay of 0 and the whole domain the meeting is a's crossing."""
    n = len(a[0])
    return [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.asarray(a[6]).copy(), np.asarray(a[7]).copy()]


def hand_made():
    """(A, B, level, lo, hi, delay, time): eight one-query problems in dyadic numbers and small integers, every breakpoint and value exact
    in float64 (the first three are gap_ref.knot_cases' 0, 1 and 2 with the level their extreme gap, which sits on a breakpoint).
      0  the meeting exactly on k_A = 1: the gap falls to -8 there and rises again.
      1  the meeting on k_B = delay + duration0_B = 1.25 with a delay of 0.25: the gap rises to 6 there.
      2  the level is the gap at the clamped start: the time carries the delay's bits, 0.5.
      3  problem 2 with lo = 0.75 and the level the gap there, -47.265625: the time carries lo's bits.
      4 - 6  a vehicle against itself 25 lower, no delay, level 25: the gap is 25 at every time and the time is a for every window --
         lo = 0.375; the clamp +0.0 of the whole domain; lo = 2.5, in segment 1.
      7  the same with level 24: never."""
    ka, kb, _, _, kd, want = gr.knot_cases()
    rows = [([x[i] for x in ka], [x[i] for x in kb], want[i][1], -np.inf, np.inf, kd[i, 0], want[i][2]) for i in range(3)]
    fall, rise = rows[2][0], rows[2][1]
    rows.append((fall, rise, -47.265625, 0.75, np.inf, 0.5, 0.75))
    drive = [0.0, 64.0, 128.0, 0.0, 0.0, 48.0, 2.0, 2.0]
    lower = [-25.0, 39.0, 103.0] + drive[3:]
    rows.append((drive, lower, 25.0, 0.375, 3.0, 0.0, 0.375))
    rows.append((drive, lower, 25.0, -np.inf, np.inf, 0.0, 0.0))
    rows.append((drive, lower, 25.0, 2.5, np.inf, 0.0, 2.5))
    rows.append((drive, lower, 24.0, 0.375, 3.0, 0.0, np.nan))
    a = [np.array([r[0][f] for r in rows], dtype=np.float64) for f in range(8)]
    b = [np.array([r[1][f] for r in rows], dtype=np.float64) for f in range(8)]
    col = lambda at: np.array([[r[at]] for r in rows], dtype=np.float64)      # noqa: E731
    return a, b, col(2), col(3), col(4), col(5), col(6)
