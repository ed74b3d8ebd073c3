"""Test-side restatements of the extreme gap between two splines (rp_trajectory_gap, csrc/trajectory.hip), on top of
tests/trajectory_ref.py and tests/extrema_ref.py: a spline is its list of eight arrays, a query a window lo, hi and a delay, three (n, k)
arrays (None: -inf / +inf / 0).  D(t) = pos_A(t) - pos_B(t - delay); the two outputs are NAMES = (gap_min, gap_max).

    candidates_ld    the definition's candidate list in longdouble with true divisions: the eleven times (n, k) in time order, whether each
                     takes part, and the value there (trajectory_ref.forward_ld of A at that time minus that of B at time - delay)
    gap_ld           the definition: the strict walk over candidates_ld; (values, times), two (n, k) longdouble arrays each
    gap_f64          the kernel's rule in float64, operation for operation (the pieces' quadratics through the kernel's formula, values
                     through trajectory_ref.forward_f64; 1 / h is numpy's division where the kernel has its refined reciprocal, so it
                     restates the rule, not the bits)
    classes          the class of each returned time by equality, in the torch layer's priority
    derivative_ld / derivative_jvp_ld
                     the documented routing on trajectory_ref.vjp_ld / jvp_ld of each spline at the returned times
    runner_up_gap    per query and output, how far the best candidate beats every candidate at a different time, in units of the scale
    pairs, delays, windows, knot_cases
                     the test inputs
"""
import numpy as np

import extrema_ref as xr
import trajectory_ref as tr

LD = np.longdouble
NAMES = ("gap_min", "gap_max")
LO, HI, END_A, END_B, KNOT_A, KNOT_B, START, INTERIOR, NONE = range(9)


def scale(a, b):
    """The position scale of a pair, (n, 1): the larger of the two splines' (trajectory_ref.scales)."""
    return np.maximum(tr.scales(a)[0], tr.scales(b)[0])


def _queries(a, lo, hi, delay, k=None):
    """(lo, hi, delay) as float64 (n, k) arrays: None is -inf / +inf / 0, all None one whole-domain query per problem."""
    n = len(a[0])
    given = next((x for x in (lo, hi, delay) if x is not None), None)
    shape = (n, 1 if k is None else k) if given is None else np.shape(given)
    lo = np.full(shape, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(shape, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    delay = np.zeros(shape) if delay is None else np.asarray(delay, dtype=np.float64)
    return lo, hi, delay


def _domain(a, b, delay):
    """The float64 times the definition is made of, (n, k) or (n, 1) each: S, E, k_A, k_B, T_A and delay + T_B."""
    pa, pb = tr._columns(a, np.float64), tr._columns(b, np.float64)
    with np.errstate(all="ignore"):
        TA, EB = pa[6] + pa[7], delay + (pb[6] + pb[7])
        kA, kB = pa[6], delay + pb[6]
        S = np.where(delay > 0, delay, 0.0)
        E = np.where(EB < TA, EB, np.broadcast_to(TA, EB.shape))
    return S, E, kA, kB, TA, EB


def _segments(spline, T):
    """Per segment (x0, va, acc0, jrk0) as (n, 1) columns of type T: the definition's true divisions in longdouble, the kernel's staged
    constants in float64."""
    if T is LD:
        p0, p1, p2, v0, v2, v1, d0, d1 = tr._columns(spline, LD)
        out = []
        with np.errstate(all="ignore"):
            for x0, x1, va, vb, h in ((p0, p1, v0, v1, d0), (p1, p2, v1, v2, d1)):
                acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
                out.append((x0, va, acc0, 2 * (vb - va) / h**2 - 2 * acc0 / h))
        return out
    sa, sb, _ = tr._staged_f64(spline)
    return [(s[0], s[2], s[4], s[5]) for s in (sa, sb)]


def _motion(segs, seg, s, T):
    """(vel, acc, jrk0) of the selected segment at local time s, in the evaluator's expressions."""
    va, acc0, jrk0 = (np.where(seg, segs[1][i], segs[0][i]) for i in (1, 2, 3))
    return va + (acc0 + jrk0 * (s * T(0.5))) * s, acc0 + jrk0 * s, jrk0 + 0 * s


def _candidates(a, b, lo, hi, delay, T):
    forward = tr.forward_ld if T is LD else tr.forward_f64
    lo, hi, delay = _queries(a, lo, hi, delay)
    S, E, kA, kB, _, EB = _domain(a, b, delay)
    S, E, kA, kB, lo, hi, dl = (np.asarray(x).astype(T) for x in (S, E, kA, kB, lo, hi, delay))
    sa, sb = _segments(a, T), _segments(b, T)
    nan = T(np.nan)
    with np.errstate(all="ignore"):
        lo_a = np.where(lo > S, lo, np.where(np.isnan(lo), lo, S))
        hi_b = np.where(hi < E, hi, np.where(np.isnan(hi), hi, E))
        ok = (lo_a <= hi_b) & np.isfinite(delay) & ~np.isnan(EB)
        wide = lambda t: np.broadcast_to(t, lo_a.shape)      # noqa: E731
        b_first = wide(kB < kA)
        knots = [np.where(b_first, wide(kB), wide(kA)), np.where(b_first, wide(kA), wide(kB))]
        times, valid = [lo_a], [ok]
        c = lo_a
        for piece in range(3):
            knot = knots[min(piece, 1)]
            e = hi_b if piece == 2 else np.where(knot < lo_a, lo_a, np.where(knot > hi_b, hi_b, knot))
            seg_a, seg_b = wide(kA <= c), wide(kB <= c)
            vel_a, acc_a, jrk_a = _motion(sa, seg_a, np.where(seg_a, c - kA, c), T)
            vel_b, acc_b, jrk_b = _motion(sb, seg_b, np.where(seg_b, c - kB, c - dl), T)
            qa, qb, qc = (jrk_a - jrk_b) * T(0.5), acc_a - acc_b, vel_a - vel_b
            disc = qb * qb - T(4) * (qa * qc)
            real = disc >= 0
            q = T(-0.5) * (qb + np.copysign(np.sqrt(np.where(real, disc, T(0))), qb))
            r0 = np.where(real & (qa != 0), q / np.where(qa != 0, qa, T(1)), nan)
            r1 = np.where(real, qc / q, nan)
            length, t0, t1 = e - c, c + r0, c + r1
            in0 = ok & (r0 > 0) & (r0 < length) & (lo_a < t0) & (t0 < hi_b)
            in1 = ok & (r1 > 0) & (r1 < length) & (lo_a < t1) & (t1 < hi_b)
            swap = in1 & (~in0 | (r1 < r0))
            times += [np.where(swap, t1, t0), np.where(swap, t0, t1)]
            valid += [np.where(swap, in1, in0), np.where(swap, in0, in1)]
            if piece < 2:
                times.append(knot)
                valid.append(ok & (lo_a <= knot) & (knot <= hi_b))
            c = e
        times.append(hi_b)
        valid.append(ok)
        values = []
        for t, v in zip(times, valid):
            at = np.where(v, t, T(0))
            values.append(forward(a, at)[0] - forward(b, np.where(v, at - dl, T(0)))[0])
    return times, valid, values


def candidates_ld(a, b, lo=None, hi=None, delay=None):
    """(times, valid, values): lists of eleven (n, k) arrays, in time order -- a, piece 0's roots, the first knot, piece 1's roots, the
    second knot, piece 2's roots, b."""
    return _candidates(a, b, lo, hi, delay, LD)


def _gap(a, b, lo, hi, delay, T):
    lo_v, lo_t, hi_v, hi_t = xr._walk(*_candidates(a, b, lo, hi, delay, T), T)
    return [lo_v, hi_v], [lo_t, hi_t]


def gap_ld(a, b, lo=None, hi=None, delay=None):
    """(values, times): two (n, k) longdouble arrays each, NAMES' order; NaN where the query has no answer."""
    return _gap(a, b, lo, hi, delay, LD)


def gap_f64(a, b, lo=None, hi=None, delay=None):
    """The same by the kernel's rule in float64."""
    return _gap(a, b, lo, hi, delay, np.float64)


def runner_up_gap(a, b, lo=None, hi=None, delay=None):
    """Two (n, k) float64 arrays: by how much of the scale the best candidate of the definition beats every candidate at a different time;
    inf where there is no other, NaN where the query has no answer."""
    times, valid, values = candidates_ld(a, b, lo, hi, delay)
    lo_v, lo_t, hi_v, hi_t = xr._walk(times, valid, values, LD)
    sc, out = scale(a, b), []
    for sign, best_v, best_t in ((1, lo_v, lo_t), (-1, hi_v, hi_t)):
        gap = np.full(best_v.shape, np.inf, dtype=LD)
        with np.errstate(all="ignore"):
            for t, ok, v in zip(times, valid, values):
                other = ok & (t != best_t) & ~np.isnan(v)
                gap = np.where(other, np.minimum(gap, sign * (v - best_v)), gap)
        out.append(np.where(np.isnan(best_v), np.nan, np.asarray(gap / sc, dtype=np.float64)))
    return out


# ---------------------------------------------------------------- derivatives: the routing
def classes(a, b, lo, hi, delay, time):
    """The class of each returned time (n, k), by equality and in this priority: LO (time == lo), HI (== hi), END_A (== T_A), END_B
    (== delay + T_B), KNOT_A (== k_A), KNOT_B (== k_B), START (== delay and delay > 0), else INTERIOR (a clamped +0.0 or a stationary point);
    NONE where it is NaN."""
    lo, hi, delay = _queries(a, lo, hi, delay, np.shape(time)[1])
    _, _, kA, kB, TA, EB = _domain(a, b, delay)
    t = np.asarray(time)
    out = np.full(t.shape, INTERIOR)
    with np.errstate(all="ignore"):
        out = np.where((t == delay) & (delay > 0), START, out)
        for cls, ref in ((KNOT_B, kB), (KNOT_A, kA), (END_B, EB), (END_A, TA), (HI, hi), (LO, lo)):      # the last one written wins
            out = np.where(t == ref, cls, out)
    return np.where(np.isnan(t.astype(np.float64)), NONE, out)


def _side_by_side(a, b, lo, hi, delay, times, values):
    """k; A's times [t_min | t_max] and B's (those minus the delay, in the times' own type), 0 where there is no value; where; the classes"""
    k = np.shape(times[0])[1]
    _, _, dl = _queries(a, lo, hi, delay, k)
    tau = np.concatenate([np.asarray(t) for t in times], axis=1)
    missing = np.isnan(tau.astype(np.float64)) | np.isnan(np.concatenate([np.asarray(v, dtype=np.float64) for v in values], axis=1))
    cls = np.where(missing, NONE, np.concatenate([classes(a, b, lo, hi, delay, t) for t in times], axis=1))
    with np.errstate(all="ignore"):
        shifted = tau - np.tile(dl, (1, 2))
    return k, np.where(missing, LD(0), tau.astype(LD)), np.where(missing, LD(0), shifted.astype(LD)), missing, cls


def derivative_ld(a, b, lo, hi, delay, times, values, g, vjp=tr.vjp_ld):
    """Reverse mode in longdouble (vjp=trajectory_ref.vjp_f64: with the evaluator's float64 restatement) at the times given: (A's eight
    gradients, B's eight, lo_bar, hi_bar, delay_bar (n, k) each) for the upstream gradients g (two (n, k) arrays).  One evaluator VJP on A
    at [t_min | t_max] with g_pos = g and one on B at those times minus the delay with g_pos = -g, 0 where the value is NaN; every finite
    query sends -tau_bar_B to delay_bar; tau_bar_A + tau_bar_B goes where the class says."""
    k, tau_a, tau_b, missing, cls = _side_by_side(a, b, lo, hi, delay, times, values)
    gp = np.where(missing, LD(0), np.concatenate([np.asarray(x, dtype=LD) for x in g], axis=1))
    zero = np.zeros(tau_a.shape, dtype=LD)
    bars_a, tb_a = vjp(a, tau_a, gp, zero, zero)
    bars_b, tb_b = vjp(b, tau_b, -gp, zero, zero)
    time_bar = tb_a + tb_b
    routed = lambda *cs: np.where(np.isin(cls, cs), time_bar, LD(0))      # noqa: E731
    fold = lambda x: x.reshape(len(x), 2, k).sum(axis=1)      # noqa: E731
    bars_a, bars_b = list(bars_a), list(bars_b)
    bars_a[6] = bars_a[6] + routed(END_A, KNOT_A).sum(axis=1)
    bars_a[7] = bars_a[7] + routed(END_A).sum(axis=1)
    bars_b[6] = bars_b[6] + routed(END_B, KNOT_B).sum(axis=1)
    bars_b[7] = bars_b[7] + routed(END_B).sum(axis=1)
    delay_bar = fold(routed(END_B, KNOT_B, START) - np.where(missing, LD(0), tb_b))
    return bars_a, bars_b, fold(routed(LO)), fold(routed(HI)), delay_bar


def derivative_jvp_ld(a, b, lo, hi, delay, times, values, a_dot, b_dot, lo_dot, hi_dot, delay_dot, jvp=tr.jvp_ld):
    """Forward mode in longdouble (jvp=trajectory_ref.jvp_f64: the float64 restatement): the two value tangents (n, k), NaN where the value
    is.  One evaluator JVP on each spline at the same times, tau_dot from the class table, B's minus delay_dot."""
    k, tau_a, tau_b, missing, cls = _side_by_side(a, b, lo, hi, delay, times, values)
    two = lambda x: np.tile(np.asarray(x, dtype=LD), (1, 2))      # noqa: E731
    col = lambda x: np.asarray(x, dtype=LD)[:, None] + np.zeros(tau_a.shape, dtype=LD)      # noqa: E731
    dd = two(delay_dot)
    time_dot = np.select([cls == LO, cls == HI, cls == END_A, cls == END_B, cls == KNOT_A, cls == KNOT_B, cls == START],
                         [two(lo_dot), two(hi_dot), col(a_dot[6]) + col(a_dot[7]), dd + col(b_dot[6]) + col(b_dot[7]), col(a_dot[6]),
                          dd + col(b_dot[6]), dd], LD(0))
    pa = jvp(a, tau_a, a_dot, time_dot)[0]
    pb = jvp(b, tau_b, b_dot, time_dot - dd)[0]
    out = np.where(missing, LD(np.nan), pa - pb)
    return [out[:, :k], out[:, k:]]


# ---------------------------------------------------------------- inputs
def random_pair(n):
    return tr.random_states(n, 1), tr.random_states(n, 2)


def solved_pair(n):
    """Problems [0, n) against [n, 2 n) of tests/golden/f3_batch.npz as the gated solve left them."""
    both = xr.solved_golden(2 * n)
    assert len(both[0]) == 2 * n
    return [x[:n].copy() for x in both], [x[n:].copy() for x in both]


def follower(a, by=25.0):
    """The same spline with its three positions lowered: with a delay of 0 the gap is `by` at every time."""
    return [x - by for x in a[:3]] + [x.copy() for x in a[3:]]


def delays(a, b, k, seed, follow=False):
    """(n, k): U(-0.3, 0.3) min(T_A, T_B), columns 0 and 2 exactly 0; follow: U(0.02, 0.3) T_A in every column."""
    rng = np.random.default_rng(seed)
    T = np.minimum(a[6] + a[7], b[6] + b[7])[:, None]
    if follow:
        return np.ascontiguousarray(rng.uniform(0.02, 0.3, (len(T), k)) * T)
    d = rng.uniform(-0.3, 0.3, (len(T), k)) * T
    d[:, 0] = 0.0
    if k > 2:
        d[:, 2] = 0.0
    return np.ascontiguousarray(d)


def windows(a, b, delay, seed):
    """(lo, hi), the delay's shape: columns 0 and 1 the whole common domain, (-inf, +inf); the others the sorted pair of two U(-0.1, 1.1)
    draws across [S, E] -- both before S or both after E about once in a hundred: the NaN rule."""
    rng = np.random.default_rng(seed)
    delay = np.asarray(delay, dtype=np.float64)
    S, E, _, _, _, _ = _domain(a, b, delay)
    draws = np.sort(rng.uniform(-0.1, 1.1, delay.shape + (2,)), axis=2)
    lo, hi = S + draws[:, :, 0] * (E - S), S + draws[:, :, 1] * (E - S)
    lo[:, :2], hi[:, :2] = -np.inf, np.inf
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def knot_cases():
    """(A, B, lo (4, 1), hi, delay, [(output, value, time, class)]): four hand-made problems in dyadic numbers and small integers, every
    constant, root and value exact in float64, one whole-domain query each.
      0  A accelerates (4 t^2), B runs at a constant 8 and started 0.5 earlier: the gap's minimum -8 is where the velocities meet, at
         t = 1 = k_A exactly -- a root of the relative velocity that sits on the ends of two pieces and is strictly inside neither.
      1  the mirror image with a delay of 0.25: the maximum 6 at t = 1.25 = k_B = delay + duration0_B.
      2  A falls, B rises from rest 0.5 later: the maximum -15.625 at the START t = delay.
      3  A rises, B falls and ends first: the maximum 187.5 at END_B, t = delay + T_B = 2.5, before T_A = 4."""
    rows = [
        # A: pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1 | B: the same | delay | output, value, time, class
        ((0.0, 4.0, 16.0, 0.0, 16.0, 8.0, 1.0, 1.0), (0.0, 16.0, 24.0, 8.0, 8.0, 8.0, 2.0, 1.0), -0.5, (0, -8.0, 1.0, KNOT_A)),
        ((0.0, 8.0, 16.0, 8.0, 8.0, 8.0, 1.0, 1.0), (0.0, 4.0, 16.0, 0.0, 16.0, 8.0, 1.0, 1.0), 0.25, (1, 6.0, 1.25, KNOT_B)),
        ((0.0, -50.0, -100.0, 0.0, 0.0, -75.0, 1.0, 1.0), (0.0, 100.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0), 0.5, (1, -15.625, 0.5, START)),
        ((0.0, 64.0, 128.0, 0.0, 0.0, 48.0, 2.0, 2.0), (0.0, -50.0, -100.0, 0.0, 0.0, -75.0, 1.0, 1.0), 0.5, (1, 187.5, 2.5, END_B)),
    ]
    a = [np.array([r[0][f] for r in rows], dtype=np.float64) for f in range(8)]
    b = [np.array([r[1][f] for r in rows], dtype=np.float64) for f in range(8)]
    delay = np.array([[r[2]] for r in rows], dtype=np.float64)
    return a, b, np.full((len(rows), 1), -np.inf), np.full((len(rows), 1), np.inf), delay, [r[3] for r in rows]
