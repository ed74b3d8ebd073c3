"""Test-side restatements of the closest approach of two vehicles moving in d axes (rp_trajectory_separation, csrc/trajectory.hip; DESIGN.md
section 24), on top of tests/trajectory_ref.py and tests/gap_ref.py.  A vehicle is a list of d splines (each a list of eight arrays of n
values, the C ABI's order), a query a window lo, hi and a delay, three (n, k) arrays (None: -inf / +inf / 0).  D_c(t) = pos_Ac(t) -
pos_Bc(t - delay), f(t) = the sum over the axes of D_c(t)^2; the outputs are the least f over the clamped window and when it is attained.

    candidates_ld    the definition's candidate list in longdouble: per piece the longdouble quintic g = f' / 2, its changes of sign on a
                     4,001-point grid refined by 120 bisections; the times in time order, whether each takes part, and f there
                     (trajectory_ref.forward_ld per axis)
    separation_ld    the definition: the strict walk over candidates_ld; (value, time), two (n, k) longdouble arrays
    separation_f64   the kernel's rule in float64, operation for operation (values through trajectory_ref.forward_f64; 1 / x is numpy's
                     division where the kernel has its refined reciprocal, so it restates the rule, not the bits), with the search trips
                     per query: (value, time, trips)
    classes          the class of each returned time by equality, in the torch layer's priority, and the axis of an END
    derivative_ld / derivative_jvp_ld
                     the documented routing on trajectory_ref.vjp_ld / jvp_ld of each spline at the returned times
    runner_up        per query, by how much of the scale^2 the best candidate of the definition beats every candidate at a different time
    family, delays, windows, hand_made
                     the test inputs
"""
import numpy as np

import extrema_ref as xr
import gap_ref as gr
import trajectory_ref as tr

LD = np.longdouble
TRIPS = 64                      # the kernel's kSepTrips
TOL = 2.0 * 2.220446049250313e-16
GRID, BISECTIONS = 4001, 120
LO, HI, END_A, END_B, START, OTHER, NONE = range(7)


def scales(a, b):
    """Per axis the position scale of the pair (gap_ref.scale), (n, 1) each, and the sum of their squares."""
    per_axis = [gr.scale(x, y) for x, y in zip(a, b)]
    return per_axis, sum(s * s for s in per_axis)


def value_bound(a, b, gaps):
    """B(t) = the sum over the axes of 2 |D_c(t)| e_c + e_c^2 with e_c = 2e-13 of axis c's scale: what float64 may move one candidate's
    value by (section 18's bound on one D_c, squared out).  gaps: the d arrays D_c at the time."""
    per_axis, _ = scales(a, b)
    return sum(2 * np.abs(np.asarray(g, dtype=np.float64)) * (2e-13 * s) + (2e-13 * s) ** 2 for g, s in zip(gaps, per_axis))


def _queries(a, lo, hi, delay, k=None):
    return gr._queries(a[0], lo, hi, delay, k)


def _domain(a, b, delay):
    """The float64 times the definition is made of: S, E (n, k), the lists k_A, k_B, T_A, E_B per axis ((n, 1) or (n, k)), and whether
    none of the 2 d splines is under the NaN rule."""
    d = len(a)
    ca, cb = [tr._columns(x, np.float64) for x in a], [tr._columns(x, np.float64) for x in b]
    with np.errstate(all="ignore"):
        TA = [c[6] + c[7] for c in ca]
        EB = [delay + (c[6] + c[7]) for c in cb]
        kA = [c[6] for c in ca]
        kB = [delay + c[6] for c in cb]
        S = np.where(delay > 0, delay, 0.0)
        E = np.full(np.shape(delay), np.inf)
        whole = np.ones(np.shape(delay), dtype=bool)
        for x in range(d):
            whole &= ~np.isnan(TA[x] + 0 * delay)
            E = np.where(TA[x] < E, TA[x], E)
        for x in range(d):
            whole &= ~np.isnan(EB[x])
            E = np.where(EB[x] < E, EB[x], E)
    return S, E, kA, kB, TA, EB, whole


def _cubic(c, s, T):
    x0, va, acc0, jrk0 = c
    third = T(1) / T(3)
    return (x0 + (va + (acc0 + jrk0 * (s * third)) * (s * T(0.5))) * s, va + (acc0 + jrk0 * (s * T(0.5))) * s, acc0 + jrk0 * s, jrk0 + 0 * s)


def _poly_at(p, u):
    v = p[-1]
    for i in range(len(p) - 2, -1, -1):
        v = p[i] + u * v
    return v


def _poly_slope(p, u, T):
    n = len(p)
    v = T(n - 1) * p[n - 1]
    for i in range(n - 2, 0, -1):
        v = T(i) * p[i] + u * v
    return v


def _search(p, lo, hi, p_lo, p_hi, tol, on):
    """poly_search, lane by lane: the point of smallest |p| looked at, and the trips made (0 where `on` is not set)."""
    T = np.float64
    up = p_lo < 0
    width = hi - lo
    best = np.where(np.abs(p_hi) < np.abs(p_lo), hi, lo)
    best_p = np.fmin(np.abs(p_lo), np.abs(p_hi))
    s = lo + width * (p_lo * (1.0 / (p_lo - p_hi)))
    s = np.where((s > lo) & (s < hi), s, lo + 0.5 * width)
    dx_old, dx = width, width
    trips = np.zeros(np.shape(s), dtype=np.int64)
    live = on.copy()
    for _ in range(TRIPS):
        if not live.any():
            break
        g, v = _poly_at(p, s), _poly_slope(p, s, T)
        trips += live
        better = live & (np.abs(g) < best_p)
        best_p, best = np.where(better, np.abs(g), best_p), np.where(better, s, best)
        live = live & ~(g == 0)
        rising = (g < 0) == up
        lo, hi = np.where(live & rising, s, lo), np.where(live & ~rising, s, hi)
        width = np.where(live, hi - lo, width)
        live = live & (width > tol)
        step = g * (1.0 / v)
        nxt = s - step
        newton = (nxt > lo) & (nxt < hi) & (2.0 * np.abs(step) <= np.abs(dx_old))
        nxt = np.where(newton, nxt, lo + 0.5 * width)
        dx_old, dx = np.where(live, dx, dx_old), np.where(live, nxt - s, dx)
        live = live & (np.abs(dx) > tol)
        s = np.where(live, nxt, s)
    return best, trips


def _roots_between(p, brk, length, tol):
    """roots_between: one root per bracket (NaN: none), the trips of all its searches and those of the longest one."""
    lo, p_lo = np.zeros(np.shape(length)), p[0] + 0 * length
    out, trips, deepest = [], 0, 0
    for j in range(len(brk) + 1):
        hi = np.where(np.isnan(brk[j]), lo, brk[j]) if j < len(brk) else length
        p_hi = _poly_at(p, hi)
        cross = ((p_lo < 0) & (p_hi >= 0)) | ((p_lo > 0) & (p_hi <= 0))
        at_end = cross & (p_hi == 0)
        r, t = _search(p, lo, hi, p_lo, p_hi, tol, cross & ~at_end)
        out.append(np.where(cross, np.where(at_end, hi, r), np.nan))
        trips, deepest = trips + t, np.maximum(deepest, t)
        lo, p_lo = hi, p_hi
    return out, trips, deepest


def _velocity_breaks(va, acc0, jrk0, h):
    """csrc/trajectory.hip's velocity_breaks: the roots of va + acc0 s + (jrk0 / 2) s^2 strictly inside (0, h), padded with 0 and h."""
    a, b, c = jrk0 * 0.5, acc0, va
    disc = b * b - 4.0 * (a * c)
    real = disc >= 0
    q = -0.5 * (b + np.copysign(np.sqrt(np.where(real, disc, 0.0)), b))
    r0 = np.where(real & (a != 0), q / np.where(a != 0, a, 1.0), np.nan)
    r1 = np.where(real, c / q, np.nan)
    in0, in1 = (r0 > 0) & (r0 < h), (r1 > 0) & (r1 < h)
    both, one = in0 & in1, in0 ^ in1
    r, other = np.where(in0, r0, r1), np.where(in0, r1, r0)
    c1 = np.where(both, np.where(r0 < r1, r0, r1), np.where(one & ~(other <= 0), r, 0.0))
    c2 = np.where(both, np.where(r0 < r1, r1, r0), np.where(one & (other <= 0), r, h))
    return c1, c2


def _quintic(a, b, segs_a, segs_b, kA, kB, dl, c, T):
    """The six coefficients of g(u) = the sum of D_c(u) D_c'(u) on the piece that starts at c, in the kernel's order of operations."""
    g = None
    for x in range(len(a)):
        seg_a, seg_b = kA[x] <= c, kB[x] <= c
        ca = [np.where(seg_a, segs_a[x][1][i], segs_a[x][0][i]) for i in range(4)]
        cb = [np.where(seg_b, segs_b[x][1][i], segs_b[x][0][i]) for i in range(4)]
        sa, sb = _cubic(ca, np.where(seg_a, c - kA[x], c), T), _cubic(cb, np.where(seg_b, c - kB[x], c - dl), T)
        X, V, A, J = (p - q for p, q in zip(sa, sb))
        p0, p1, p2, p3 = X, V, A * T(0.5), J * (T(1) / T(6))
        q0, q1, q2 = V, A, J * T(0.5)
        t = [p0 * q0, p0 * q1 + p1 * q0, (p0 * q2 + p1 * q1) + p2 * q0, (p1 * q2 + p2 * q1) + p3 * q0, p2 * q2 + p3 * q1, p3 * q2]
        g = [T(0) + v for v in t] if g is None else [u + v for u, v in zip(g, t)]      # the kernel's sums start from 0.0
    return g


def _value(a, b, t, dl, on, forward, T):
    """f at the times t (0 where `on` is not set), and the d gaps"""
    at = np.where(on, t, T(0))
    gaps = [forward(x, at)[0] - forward(y, np.where(on, at - dl, T(0)))[0] for x, y in zip(a, b)]
    total = None
    for gap in gaps:
        total = gap * gap if total is None else total + gap * gap
    return total, gaps


def _setup(a, b, lo, hi, delay, T):
    lo, hi, delay = _queries(a, lo, hi, delay)
    S, E, kA, kB, _, _, whole = _domain(a, b, delay)
    with np.errstate(all="ignore"):
        wa = np.where(lo > S, lo, np.where(np.isnan(lo), lo, S))
        wb = np.where(hi < E, hi, np.where(np.isnan(hi), hi, E))
        ok = (wa <= wb) & np.isfinite(delay) & whole
    wide = lambda t: np.broadcast_to(np.asarray(t).astype(T), wa.shape)      # noqa: E731
    return wa.astype(T), wb.astype(T), ok, [wide(x) for x in kA], [wide(x) for x in kB], delay.astype(T)


def _piece_end(c, wb, kA, kB):
    e = wb
    for x in range(len(kA)):
        e = np.where((kA[x] > c) & (kA[x] < e), kA[x], e)
        e = np.where((kB[x] > c) & (kB[x] < e), kB[x], e)
    return e


def _candidates_f64(a, b, lo, hi, delay):
    T = np.float64
    wa, wb, ok, kA, kB, dl = _setup(a, b, lo, hi, delay, T)
    segs_a, segs_b = [gr._segments(x, T) for x in a], [gr._segments(x, T) for x in b]
    times, valid, trips, deepest = [wa], [ok], np.zeros(wa.shape, dtype=np.int64), np.zeros(wa.shape, dtype=np.int64)
    c = wa
    with np.errstate(all="ignore"):
        for _ in range(2 * len(a) + 1):
            e = _piece_end(c, wb, kA, kB)
            g = _quintic(a, b, segs_a, segs_b, kA, kB, dl, c, T)
            length, tol = e - c, TOL * e
            g1 = [g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4], 5.0 * g[5]]
            g2 = [2.0 * g[2], 6.0 * g[3], 12.0 * g[4], 20.0 * g[5]]
            r3 = _velocity_breaks(6.0 * g[3], 24.0 * g[4], 120.0 * g[5], length)
            r2, t2, m2 = _roots_between(g2, list(r3), length, tol)
            r1, t1, m1 = _roots_between(g1, r2, length, tol)
            r0, t0, m0 = _roots_between(g, r1, length, tol)
            trips, deepest = trips + t2 + t1 + t0, np.maximum(np.maximum(deepest, m2), np.maximum(m1, m0))
            for u in r0:
                t = c + u
                times.append(t)
                valid.append(ok & (u > 0) & (u < length) & (wa < t) & (t < wb))
            times.append(e)
            valid.append(ok & (e < wb))
            c = e
    times.append(wb)
    valid.append(ok)
    values = [_value(a, b, t, dl, v, tr.forward_f64, T)[0] for t, v in zip(times, valid)]
    return times, valid, values, trips, deepest


def _grid_roots(g, length):
    """The changes of sign of the longdouble quintic g on (0, length] (arrays of m pieces): a list of (piece index, root) arrays, every
    change of sign on the 4,001-point grid refined by 120 bisections; a grid point where g is exactly 0 is the root itself."""
    m = len(length)
    rows, roots = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=LD)]
    u = np.linspace(0.0, 1.0, GRID).astype(LD)
    for first in range(0, m, 512):
        part = slice(first, min(first + 512, m))
        gp = [x[part, None] for x in g]
        ln = length[part, None]
        at = u[None, :] * ln
        at[:, -1] = ln[:, 0]
        v = _poly_at(gp, at)
        cross = ((v[:, :-1] < 0) & (v[:, 1:] >= 0)) | ((v[:, :-1] > 0) & (v[:, 1:] <= 0))
        r, j = np.nonzero(cross)
        lo, hi = at[r, j], at[r, j + 1]
        p_lo, p_hi = v[r, j], v[r, j + 1]
        coeff = [x[part][r] for x in g]
        done = p_hi == 0
        lo = np.where(done, hi, lo)
        for _ in range(BISECTIONS):
            mid = lo + (hi - lo) * LD(0.5)
            pm = _poly_at(coeff, mid)
            zero = pm == 0
            left = ((pm < 0) == (p_lo < 0)) & ~zero
            lo = np.where(done, lo, np.where(zero | left, mid, lo))
            hi = np.where(done, hi, np.where(zero | ~left, mid, hi))
        rows.append(r + first)
        roots.append(np.where(done, hi, lo + (hi - lo) * LD(0.5)))
    return np.concatenate(rows), np.concatenate(roots)


def _candidates_ld(a, b, lo, hi, delay):
    wa, wb, ok, kA, kB, dl = _setup(a, b, lo, hi, delay, LD)
    segs_a, segs_b = [gr._segments(x, LD) for x in a], [gr._segments(x, LD) for x in b]
    times, valid = [wa], [ok]
    c = wa
    with np.errstate(all="ignore"):
        for _ in range(2 * len(a) + 1):
            e = _piece_end(c, wb, kA, kB)
            g = _quintic(a, b, segs_a, segs_b, kA, kB, dl, c, LD)
            length = e - c
            live = ok & (length > 0)
            where = np.nonzero(live.ravel())[0]
            piece, root = _grid_roots([np.broadcast_to(x, wa.shape).ravel()[where] for x in g], length.ravel()[where])
            # a quintic has five roots at the most; the slots are filled in time order (the grid's)
            slot = np.zeros(len(piece), dtype=np.int64)
            if len(piece):
                same = np.concatenate([[False], piece[1:] == piece[:-1]])
                for i in range(1, len(piece)):
                    slot[i] = slot[i - 1] + 1 if same[i] else 0
            for s in range(int(slot.max()) + 1 if len(piece) else 0):
                u = np.full(wa.size, np.nan, dtype=LD)
                u[where[piece[slot == s]]] = root[slot == s]
                u = u.reshape(wa.shape)
                t = c + u
                times.append(t)
                valid.append(ok & (u > 0) & (u < length) & (wa < t) & (t < wb))
            times.append(e)
            valid.append(ok & (e < wb))
            c = e
    times.append(wb)
    valid.append(ok)
    values = [_value(a, b, t, dl, v, tr.forward_ld, LD)[0] for t, v in zip(times, valid)]
    return times, valid, values


def candidates_ld(a, b, lo=None, hi=None, delay=None):
    """(times, valid, values): lists of (n, k) longdouble arrays in time order."""
    return _candidates_ld(a, b, lo, hi, delay)


def _walk(times, valid, values, T):
    v, t, _, _ = xr._walk(times, valid, values, T)
    return v, t


def separation_ld(a, b, lo=None, hi=None, delay=None, candidates=None):
    """(value, time): the least squared distance and when it is attained, (n, k) longdouble each; NaN where the query has no answer."""
    return _walk(*(candidates if candidates is not None else _candidates_ld(a, b, lo, hi, delay)), LD)


def separation_f64(a, b, lo=None, hi=None, delay=None, depth=False):
    """(value, time, trips) by the kernel's rule in float64; trips: the search trips each query made, all its pieces together; depth: also
    the trips of its longest single search, the number the kernel's fixed bound holds."""
    times, valid, values, trips, deepest = _candidates_f64(a, b, lo, hi, delay)
    v, t = _walk(times, valid, values, np.float64)
    return (v, t, trips, deepest) if depth else (v, t, trips)


def f_ld(a, b, t, delay):
    """(f, the d gaps) in longdouble at the times t (n, k), wherever they lie."""
    t = np.asarray(t, dtype=LD)
    return _value(a, b, t, np.asarray(delay, dtype=LD), np.ones(t.shape, dtype=bool), tr.forward_ld, LD)


def runner_up(a, b, lo=None, hi=None, delay=None, candidates=None, unit="position"):
    """(n, k) float64: by how much the best candidate of the definition beats every candidate at a different time; inf where there is no
    other, NaN where the query has no answer.  unit="position": in units of the positional scale^2, the sum over the axes of the squares
    of section 18's scale -- what rounding errors of f are measured in, so the unit of the 1e-9 that tells a tie from a winner.
    unit="distance": in units of the largest squared distance among the query's own candidates -- the unit of the 1e-2 that makes a
    difference quotient a yardstick.  f is quadratic where section 18's gap is linear: vehicles 25 apart at coordinates of 2,000 have
    f of 1e3 .. 1e4 against a positional scale^2 of 7e6, of which no candidate can lead by a hundredth; a step of 1e-6 of an input
    moves f by 2 |D| 1e-6 scale, four orders below a hundredth of f only where f is measured in its own size."""
    times, valid, values = candidates if candidates is not None else _candidates_ld(a, b, lo, hi, delay)
    best_v, best_t = _walk(times, valid, values, LD)
    gap = np.full(best_v.shape, np.inf, dtype=LD)
    most = np.full(best_v.shape, -np.inf, dtype=LD)
    with np.errstate(all="ignore"):
        for t, ok, v in zip(times, valid, values):
            other = ok & (t != best_t) & ~np.isnan(v)
            gap = np.where(other, np.minimum(gap, v - best_v), gap)
            most = np.where(ok & ~np.isnan(v), np.maximum(most, v), most)
        assert unit in ("position", "distance"), unit
        per = scales(a, b)[1] if unit == "position" else np.maximum(most, LD(1e-300))
        return np.where(np.isnan(best_v), np.nan, np.asarray(gap / per, dtype=np.float64))


# ---------------------------------------------------------------- derivatives: the routing
def classes(a, b, lo, hi, delay, time):
    """(class, axis) of each returned time (n, k), by equality and in this priority: LO (time == lo), HI (== hi), END_A of axis 0, 1, ...
    (== T_Ac), END_B of axis 0, 1, ... (== delay + T_Bc), START (== delay and delay > 0), else OTHER (a stationary point, a knot, the clamp
    +0.0); NONE where it is NaN.  axis: the END's, else 0."""
    lo, hi, delay = _queries(a, lo, hi, delay, np.shape(time)[1])
    _, _, _, _, TA, EB, _ = _domain(a, b, delay)
    t = np.asarray(time)
    cls, axis = np.full(t.shape, OTHER), np.zeros(t.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        cls = np.where((t == delay) & (delay > 0), START, cls)
        for which, ends in ((END_B, EB), (END_A, TA)):      # the last one written wins
            for x in range(len(a) - 1, -1, -1):
                hit = t == ends[x]
                cls, axis = np.where(hit, which, cls), np.where(hit, x, axis)
        cls = np.where(t == hi, HI, cls)
        cls = np.where(t == lo, LO, cls)
    cls = np.where(np.isnan(t.astype(np.float64)), NONE, cls)
    return cls, np.where((cls == END_A) | (cls == END_B), axis, 0)


def _at_times(a, b, lo, hi, delay, time, value):
    k = np.shape(time)[1]
    _, _, dl = _queries(a, lo, hi, delay, k)
    missing = np.isnan(np.asarray(time, dtype=np.float64)) | np.isnan(np.asarray(value, dtype=np.float64))
    cls, axis = classes(a, b, lo, hi, delay, time)
    cls = np.where(missing, NONE, cls)
    with np.errstate(all="ignore"):
        shifted = np.asarray(time) - dl      # in the time's own type: what the device passes to B
    t_a = np.where(missing, LD(0), np.asarray(time).astype(LD))
    t_b = np.where(missing, LD(0), shifted.astype(LD))
    return t_a, t_b, missing, cls, axis


def derivative_ld(a, b, lo, hi, delay, time, value, g, vjp=tr.vjp_ld, forward=tr.forward_ld):
    """Reverse mode in longdouble (vjp=trajectory_ref.vjp_f64, forward=forward_f64: with the evaluator's float64 restatement) at the times
    given: (A's d lists of eight gradients, B's, lo_bar, hi_bar, delay_bar (n, k) each) for the upstream gradient g (n, k) on the value.
    Per axis one evaluator VJP on A_c at the time with g_pos = 2 g D_c and one on B_c at time - delay with g_pos = -2 g D_c, 0 where the
    value is NaN; every finite query sends minus the sum of tau_bar_Bc to delay_bar; the sum of all tau_bar goes where the class says."""
    t_a, t_b, missing, cls, axis = _at_times(a, b, lo, hi, delay, time, value)
    T = t_a.dtype.type
    gq = np.where(missing, LD(0), np.asarray(g, dtype=LD))
    zero = np.zeros(t_a.shape, dtype=LD)
    bars_a, bars_b, time_bar, shift_bar = [], [], zero, zero
    for x, y in zip(a, b):
        gap = np.asarray(forward(x, t_a)[0], dtype=LD) - np.asarray(forward(y, t_b)[0], dtype=LD)
        gp = 2 * gq * np.where(missing, T(0), gap)
        bar_x, tb_x = vjp(x, t_a, gp, zero, zero)
        bar_y, tb_y = vjp(y, t_b, -gp, zero, zero)
        bars_a.append([np.asarray(v, dtype=LD) for v in bar_x])
        bars_b.append([np.asarray(v, dtype=LD) for v in bar_y])
        time_bar = time_bar + np.where(missing, LD(0), tb_x) + np.where(missing, LD(0), tb_y)
        shift_bar = shift_bar + np.where(missing, LD(0), tb_y)
    for x in range(len(a)):
        end_a = np.where((cls == END_A) & (axis == x), time_bar, LD(0)).sum(axis=1)
        end_b = np.where((cls == END_B) & (axis == x), time_bar, LD(0)).sum(axis=1)
        bars_a[x][6], bars_a[x][7] = bars_a[x][6] + end_a, bars_a[x][7] + end_a
        bars_b[x][6], bars_b[x][7] = bars_b[x][6] + end_b, bars_b[x][7] + end_b
    routed = lambda *cs: np.where(np.isin(cls, cs), time_bar, LD(0))      # noqa: E731
    return bars_a, bars_b, routed(LO), routed(HI), routed(END_B, START) - shift_bar


def derivative_jvp_ld(a, b, lo, hi, delay, time, value, a_dot, b_dot, lo_dot, hi_dot, delay_dot, jvp=tr.jvp_ld, forward=tr.forward_ld):
    """Forward mode in longdouble (jvp=trajectory_ref.jvp_f64, forward=forward_f64: the float64 restatement): the value's tangent (n, k),
    NaN where the value is.  Per axis one evaluator JVP on each spline at the same times, tau_dot from the class table, B's minus
    delay_dot; the tangent is the sum of 2 D_c (pos_dot_Ac - pos_dot_Bc)."""
    t_a, t_b, missing, cls, axis = _at_times(a, b, lo, hi, delay, time, value)
    col = lambda v: np.asarray(v, dtype=LD)[:, None] + np.zeros(t_a.shape, dtype=LD)      # noqa: E731
    dd = np.asarray(delay_dot, dtype=LD)
    conds, picks = [cls == LO, cls == HI, cls == START], [np.asarray(lo_dot, dtype=LD), np.asarray(hi_dot, dtype=LD), dd]
    for x in range(len(a)):
        conds += [(cls == END_A) & (axis == x), (cls == END_B) & (axis == x)]
        picks += [col(a_dot[x][6]) + col(a_dot[x][7]), dd + col(b_dot[x][6]) + col(b_dot[x][7])]
    time_dot = np.select(conds, picks, LD(0))
    out = np.zeros(t_a.shape, dtype=LD)
    for x, y, xd, yd in zip(a, b, a_dot, b_dot):
        gap = np.asarray(forward(x, t_a)[0], dtype=LD) - np.asarray(forward(y, t_b)[0], dtype=LD)
        pa, pb = jvp(x, t_a, xd, time_dot)[0], jvp(y, t_b, yd, time_dot - dd)[0]
        out = out + 2 * gap * (np.asarray(pa, dtype=LD) - np.asarray(pb, dtype=LD))
    return np.where(missing, LD(np.nan), out)


# ---------------------------------------------------------------- inputs
def delays(a, b, k, seed, follow=False):
    """gap_ref.delays over the 2 d splines: U(-0.3, 0.3) of the smallest total time, columns 0 and 2 exactly 0; follow: U(0.02, 0.3) of it
    in every column."""
    rng = np.random.default_rng(seed)
    T = np.min([x[6] + x[7] for x in list(a) + list(b)], axis=0)[:, None]
    if follow:
        return np.ascontiguousarray(rng.uniform(0.02, 0.3, (len(T), k)) * T)
    d = rng.uniform(-0.3, 0.3, (len(T), k)) * T
    d[:, 0] = 0.0
    if k > 2:
        d[:, 2] = 0.0
    return np.ascontiguousarray(d)


def windows(a, b, delay, seed):
    """gap_ref.windows over the 2 d splines' common domain: columns 0 and 1 the whole domain, (-inf, +inf); the others the sorted pair of
    two U(-0.1, 1.1) draws across [S, E] -- both before S or both after E about once in a hundred: the NaN rule."""
    rng = np.random.default_rng(seed)
    delay = np.asarray(delay, dtype=np.float64)
    S, E = _domain(a, b, delay)[:2]
    draws = np.sort(rng.uniform(-0.1, 1.1, delay.shape + (2,)), axis=2)
    lo, hi = S + draws[:, :, 0] * (E - S), S + draws[:, :, 1] * (E - S)
    lo[:, :2], hi[:, :2] = -np.inf, np.inf
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def vehicles(name, n, d):
    """(A, B) of a family: random -- axis c of A is random_states(n, 1 + 2 c), of B random_states(n, 2 + 2 c); solved -- consecutive
    blocks of n problems of tests/golden/f3_batch.npz as the gated solve left them, alternating A and B per axis; follower, follower0 --
    the random A, and B the same with every position lowered by 25."""
    if name == "solved":
        every = xr.solved_golden(2 * d * n)
        assert len(every[0]) == 2 * d * n
        block = lambda j: [x[j * n:(j + 1) * n].copy() for x in every]      # noqa: E731
        return [block(2 * c) for c in range(d)], [block(2 * c + 1) for c in range(d)]
    a = [tr.random_states(n, 1 + 2 * c) for c in range(d)]
    if name == "random":
        return a, [tr.random_states(n, 2 + 2 * c) for c in range(d)]
    assert name in ("follower", "follower0"), name
    return a, [gr.follower(x) for x in a]


def family(name, n, k, d, seed=7):
    """(A, B, lo, hi, delay) of a family; follower: delays U(0.02, 0.3) T; follower0: no delay, where f is structurally 625 d."""
    a, b = vehicles(name, n, d)
    delay = np.zeros((n, k)) if name == "follower0" else delays(a, b, k, seed + d, follow=name == "follower")
    lo, hi = windows(a, b, delay, seed + 10 + d)
    return a, b, lo, hi, delay


def hand_made():
    """(A, B, lo (4, 1), hi, delay, [(value, time, class, axis)]): four hand-made problems of d = 2 in dyadic numbers and small integers,
    every constant, root and value exact in float64, one whole-domain query each.  On axis 0 both vehicles run at the same constant
    velocity 2, so D_0 is a constant and f = D_0^2 + D_1^2 is least where |D_1| is:
      0  axis 1: A is 4 t^2 + 40, B runs at a constant 8 and started 0.5 earlier: D_1 = 4 t^2 - 8 t + 36 is least, 32, at t = 1 = k_A1
         exactly -- a root of g that sits on the ends of two pieces and is strictly inside neither; D_0 = 3.
      1  axis 1: A falls, B rises from rest 0.5 later (gap_ref.knot_cases' case 2): D_1 <= -15.625, reached at the START t = delay; D_0 = 4.
      2  axis 1: A rises from rest, B stands at 1000: D_1 < 0 shrinks until the window ends, at END_B of axis 0, delay + T_B0 = 2, before
         every other end; D_1 = 64 - 1000 there; D_0 = 4.
      3  axis 1: A is 4 t^2 + 34, B runs at a constant 4 from 2, no delay: D_1 = 4 t^2 - 4 t + 32, D_1' = 8 t - 4 has its root at t = 0.5,
         strictly inside the first piece [0, 1], where D_1 = 31; g's end values there are -128 and 128, so the search's secant start is
         the root itself; D_0 = 3."""
    rest = lambda p0, p1, p2, d0, d1, v1: (p0, p1, p2, 0.0, 0.0, v1, d0, d1)      # noqa: E731
    line = lambda p0, v, d0, d1: (p0, p0 + v * d0, p0 + v * (d0 + d1), v, v, v, d0, d1)      # noqa: E731
    rows = [
        # A_0, B_0, A_1, B_1, delay, (value, time, class, axis)
        (line(3.0, 2.0, 0.5, 2.0), line(-1.0, 2.0, 1.0, 2.0), (40.0, 44.0, 56.0, 0.0, 16.0, 8.0, 1.0, 1.0), line(0.0, 8.0, 2.0, 1.0), -0.5,
         (9.0 + 32.0 ** 2, 1.0, OTHER, 0)),
        (line(3.0, 2.0, 0.5, 2.0), line(0.0, 2.0, 1.0, 2.0), rest(0.0, -50.0, -100.0, 1.0, 1.0, -75.0), rest(0.0, 100.0, 0.0, 1.0, 1.0, 0.0), 0.5,
         (16.0 + 15.625 ** 2, 0.5, START, 0)),
        (line(3.0, 2.0, 2.0, 2.0), line(0.0, 2.0, 0.5, 1.0), rest(0.0, 64.0, 128.0, 2.0, 2.0, 48.0), line(1000.0, 0.0, 2.0, 2.0), 0.5,
         (16.0 + 936.0 ** 2, 2.0, END_B, 0)),
        (line(3.0, 2.0, 1.0, 2.0), line(0.0, 2.0, 1.0, 2.0), (34.0, 38.0, 50.0, 0.0, 16.0, 8.0, 1.0, 1.0), line(2.0, 4.0, 2.0, 1.0), 0.0,
         (9.0 + 31.0 ** 2, 0.5, OTHER, 0)),
    ]
    pack = lambda col: [np.array([r[col][f] for r in rows], dtype=np.float64) for f in range(8)]      # noqa: E731
    a, b = [pack(0), pack(2)], [pack(1), pack(3)]
    delay = np.array([[r[4]] for r in rows], dtype=np.float64)
    return a, b, np.full((len(rows), 1), -np.inf), np.full((len(rows), 1), np.inf), delay, [r[5] for r in rows]
