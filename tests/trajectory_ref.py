"""Test-side restatements of the trajectory evaluator (rp_trajectory_eval / _vjp / _jvp, csrc/trajectory.hip).

A spline is a list of eight arrays of n values in the order of the C ABI's pointer tables,
    (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1),
and tau an (n, k) array of times from the start of segment 0.  Two restatements:

    forward_ld / vjp_ld / jvp_ld      the definition in longdouble with true divisions: the segment rule (tau < duration0: segment 0),
                                      the cubic of drawSegment (onedpath_ip.cpp:1065-1088), the reverse rule as its four sums per
                                      segment and the chain rule through (acc0, jrk0), the forward rule as the total derivative
    forward_f64 / vjp_f64 / jvp_f64   the kernels' own float64 arithmetic, operation for operation, and the VJP's summation order:
                                      G lanes per problem (G from k alone), lane l adding queries l, l + G, ... (pairs when k is even),
                                      then an xor butterfly.  (1 / h is numpy's division where the kernel's refined reciprocal is
                                      correctly rounded but for ~1e-7 of its inputs, csrc/ip_core.h.)

NaN rule in both: a problem with a duration that is not finite or not > 0 is NaN everywhere.
"""
import numpy as np

LD = np.longdouble
ORDER = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")


def spline_of_state(states, variant=3):
    """The eight spline arrays of states in the reference's AoS layout (n, 16) / (n, 12)."""
    s = np.asarray(states, dtype=np.float64)
    cb = 3 + (8 if variant == 3 else 4)
    return [s[:, cb + 0].copy(), s[:, cb + 2].copy(), s[:, cb + 3].copy(), s[:, cb + 1].copy(), s[:, cb + 4].copy(),
            s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy()]


def _columns(spline, T):
    cols = [np.asarray(a, dtype=T)[:, None] for a in spline]
    d0, d1 = cols[6], cols[7]
    bad = ~(np.isfinite(d0) & (d0 > 0) & np.isfinite(d1) & (d1 > 0))
    nan = np.where(bad, T(np.nan), T(0))
    cols[6], cols[7] = d0 + nan, d1 + nan
    return cols


def _select(cols, tau):
    """Per query: the segment (bool, True: segment 1) and its (x0, x1, va, vb, h, s)."""
    p0, p1, p2, v0, v2, v1, d0, d1 = cols
    seg = ~(tau < d0)
    w = lambda a, b: np.where(seg, b, a)      # noqa: E731
    return seg, w(p0, p1) + 0 * tau, w(p1, p2) + 0 * tau, w(v0, v1) + 0 * tau, w(v1, v2) + 0 * tau, w(d0, d1) + 0 * tau, np.where(seg, tau - d0, tau)


# ---------------------------------------------------------------- the definition, longdouble
def forward_ld(spline, tau):
    """(pos, vel, acc), each (n, k) longdouble."""
    tau = np.asarray(tau, dtype=LD)
    with np.errstate(all="ignore"):
        _, x0, x1, va, vb, h, s = _select(_columns(spline, LD), tau)
        acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
        jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
        pos = x0 + (va + (acc0 + jrk0 * s / 3) * s / 2) * s
        vel = va + (acc0 + jrk0 * s / 2) * s
        acc = acc0 + jrk0 * s
    return pos, vel, acc


def vjp_ld(spline, tau, gp, gv, ga):
    """(spline_bar: eight arrays of n, tau_bar (n, k)) in longdouble, for upstream gradients gp, gv, ga (n, k) on pos, vel, acc."""
    tau, gp, gv, ga = (np.asarray(a, dtype=LD) for a in (tau, gp, gv, ga))
    cols = _columns(spline, LD)
    with np.errstate(all="ignore"):
        seg, x0, x1, va, vb, h, s = _select(cols, tau)
        acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
        jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
        vel = va + (acc0 + jrk0 * s / 2) * s
        acc = acc0 + jrk0 * s
        tau_bar = gp * vel + gv * acc + ga * jrk0
        w = [gp, gp * s + gv, gp * s**2 / 2 + gv * s + ga, gp * s**3 / 6 + gv * s**2 / 2 + ga * s]
        p0, p1, p2, v0, v2, v1, d0, d1 = [c[:, 0] for c in cols]
        out = []
        for which, (a0, a1, ua, ub, hh) in enumerate(((p0, p1, v0, v1, d0), (p1, p2, v1, v2, d1))):
            m = seg == bool(which)
            Sx, Sv, Sa, Sj = [np.sum(np.where(m, x, LD(0)), axis=1) for x in w]
            a_0 = 6 * (a1 - a0) / hh**2 - (4 * ua + 2 * ub) / hh
            A = Sa - 2 / hh * Sj
            out.append((Sx - 6 * A / hh**2, 6 * A / hh**2, Sv - 4 * A / hh - 2 * Sj / hh**2, -2 * A / hh + 2 * Sj / hh**2,
                        A * (-12 * (a1 - a0) / hh**3 + (4 * ua + 2 * ub) / hh**2) + Sj * (-4 * (ub - ua) / hh**3 + 2 * a_0 / hh**2)))
        T1 = np.sum(np.where(seg, tau_bar, LD(0)), axis=1)
        (ax0, ax1, ava, avb, ah), (bx0, bx1, bva, bvb, bh) = out
        bad = np.isnan(d0)
        bars = [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah - T1, bh]
        bars = [np.where(bad, LD(np.nan), b) for b in bars]
    return bars, tau_bar


def jvp_ld(spline, tau, spline_dot, tau_dot):
    """(pos_dot, vel_dot, acc_dot) in longdouble for tangents on the eight inputs (arrays of n) and on tau (n, k)."""
    tau, tau_dot = np.asarray(tau, dtype=LD), np.asarray(tau_dot, dtype=LD)
    cols = _columns(spline, LD)
    dots = [np.asarray(a, dtype=LD)[:, None] for a in spline_dot]
    with np.errstate(all="ignore"):
        seg, x0, x1, va, vb, h, s = _select(cols, tau)
        w = lambda a, b: np.where(seg, b, a) + 0 * tau      # noqa: E731
        x0d, x1d, vad, vbd, hd = w(dots[0], dots[1]), w(dots[1], dots[2]), w(dots[3], dots[5]), w(dots[5], dots[4]), w(dots[6], dots[7])
        sd = np.where(seg, tau_dot - dots[6], tau_dot)
        acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
        jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
        acc0d = 6 * (x1d - x0d) / h**2 - 12 * (x1 - x0) * hd / h**3 - (4 * vad + 2 * vbd) / h + (4 * va + 2 * vb) * hd / h**2
        jrk0d = 2 * (vbd - vad) / h**2 - 4 * (vb - va) * hd / h**3 - 2 * acc0d / h + 2 * acc0 * hd / h**2
        vel = va + (acc0 + jrk0 * s / 2) * s
        acc = acc0 + jrk0 * s
        pd = x0d + (vad + (acc0d + jrk0d * s / 3) * s / 2) * s + vel * sd
        vd = vad + (acc0d + jrk0d * s / 2) * s + acc * sd
        ad = acc0d + jrk0d * s + jrk0 * sd
    return pd, vd, ad


# ---------------------------------------------------------------- the kernels' arithmetic, float64
def _constants_f64(x0, x1, va, vb, ih):
    ih2 = ih * ih
    acc0 = (x1 - x0) * (6.0 * ih2) - (va * 4.0 + vb * 2.0) * ih
    jrk0 = (vb - va) * (2.0 * ih2) - acc0 * (2.0 * ih)
    return acc0, jrk0


def _staged_f64(spline):
    """Per problem (columns of shape (n, 1)): the two segments' (x0, x1, va, vb, acc0, jrk0, ih) and duration0."""
    p0, p1, p2, v0, v2, v1, d0, d1 = _columns(spline, np.float64)
    with np.errstate(all="ignore"):
        ih0, ih1 = 1.0 / d0, 1.0 / d1
        a = (p0, p1, v0, v1) + _constants_f64(p0, p1, v0, v1, ih0) + (ih0,)
        b = (p1, p2, v1, v2) + _constants_f64(p1, p2, v1, v2, ih1) + (ih1,)
    return a, b, d0


def forward_f64(spline, tau):
    """(pos, vel, acc) float64 as k_trajectory_eval forms them."""
    tau = np.asarray(tau, dtype=np.float64)
    a, b, d0 = _staged_f64(spline)
    with np.errstate(all="ignore"):
        seg = ~(tau < d0)
        s = np.where(seg, tau - d0, tau)
        x0, va, acc0, jrk0 = (np.where(seg, b[i], a[i]) for i in (0, 2, 4, 5))
        pos = x0 + (va + (acc0 + jrk0 * (s * (1.0 / 3.0))) * (s * 0.5)) * s
        vel = va + (acc0 + jrk0 * (s * 0.5)) * s
        acc = acc0 + jrk0 * s
    return pos, vel, acc


def group_lanes(k):
    """(lanes per problem, whether a lane takes pairs) of k_trajectory_vjp: from k alone."""
    vec = k % 2 == 0
    units = k // 2 if vec else k
    G = 1
    while G < 64 and G < units:
        G *= 2
    return G, vec


def vjp_f64(spline, tau, gp, gv, ga):
    """(spline_bar: eight arrays of n, tau_bar (n, k)) float64 as k_trajectory_vjp forms them, in its order of additions."""
    tau, gp, gv, ga = (np.asarray(x, dtype=np.float64) for x in (tau, gp, gv, ga))
    n, k = tau.shape
    a, b, d0 = _staged_f64(spline)
    with np.errstate(all="ignore"):
        seg = ~(tau < d0)
        s = np.where(seg, tau - d0, tau)
        va, acc0, jrk0 = (np.where(seg, b[i], a[i]) for i in (2, 4, 5))
        vel = va + (acc0 + jrk0 * (s * 0.5)) * s
        acc = acc0 + jrk0 * s
        tau_bar = gp * vel + gv * acc + ga * jrk0
        h2 = s * (s * 0.5)
        h3 = h2 * (s * (1.0 / 3.0))
        w = [gp, gp * s + gv, gp * h2 + gv * s + ga, gp * h3 + gv * h2 + ga * s]
        terms = [np.where(seg, 0.0, x) for x in w] + [np.where(seg, x, 0.0) for x in w] + [np.where(seg, tau_bar, 0.0)]
        terms = np.stack(terms, axis=0)                      # (9, n, k)
        G, vec = group_lanes(k)
        per = 2 if vec else 1
        units = k // per
        S = np.zeros((9, n, G))
        for first in range(0, units, G):                     # a lane's units in order; within a pair, the first query first
            lanes = np.arange(min(G, units - first))
            for e in range(per):
                S[:, :, lanes] = S[:, :, lanes] + terms[:, :, (first + lanes) * per + e]
        m = 1
        while m < G:
            S = S + S[:, :, np.arange(G) ^ m]
            m *= 2
        S = S[:, :, 0]
        out = []
        for which, c in enumerate((a, b)):
            xa, xb, ua, ub, a0, _, ih = (x[:, 0] for x in c)
            Sx, Sv, Sa, Sj = S[4 * which:4 * which + 4]
            dx = xb - xa
            ih2 = ih * ih
            ih3 = ih2 * ih
            A = Sa - (2.0 * ih) * Sj
            x1b = (6.0 * ih2) * A
            out.append((Sx - x1b, x1b, Sv - (4.0 * ih) * A - (2.0 * ih2) * Sj, (2.0 * ih2) * Sj - (2.0 * ih) * A,
                        A * ((ua * 4.0 + ub * 2.0) * ih2 - dx * (12.0 * ih3)) + Sj * (a0 * (2.0 * ih2) - (ub - ua) * (4.0 * ih3))))
        (ax0, ax1, ava, avb, ah), (bx0, bx1, bva, bvb, bh) = out
        bars = [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah - S[8], bh]
    return bars, tau_bar


def jvp_f64(spline, tau, spline_dot, tau_dot):
    """(pos_dot, vel_dot, acc_dot) float64 as k_trajectory_jvp forms them."""
    tau, tau_dot = np.asarray(tau, dtype=np.float64), np.asarray(tau_dot, dtype=np.float64)
    a, b, d0 = _staged_f64(spline)
    d = [np.asarray(x, dtype=np.float64)[:, None] for x in spline_dot]

    def tangents(c, dxd, vad, vbd, hd):
        x0, x1, va, vb, acc0, _, ih = c
        dx = x1 - x0
        ih2 = ih * ih
        ih3 = ih2 * ih
        acc0d = dxd * (6.0 * ih2) - dx * (12.0 * ih3) * hd - (vad * 4.0 + vbd * 2.0) * ih + (va * 4.0 + vb * 2.0) * ih2 * hd
        jrk0d = (vbd - vad) * (2.0 * ih2) - (vb - va) * (4.0 * ih3) * hd - acc0d * (2.0 * ih) + acc0 * (2.0 * ih2) * hd
        return acc0d, jrk0d

    with np.errstate(all="ignore"):
        ta = (d[0], d[3]) + tangents(a, d[1] - d[0], d[3], d[5], d[6])
        tb = (d[1], d[5]) + tangents(b, d[2] - d[1], d[5], d[4], d[7])
        seg = ~(tau < d0)
        s = np.where(seg, tau - d0, tau)
        sd = np.where(seg, tau_dot - d[6], tau_dot)
        va, acc0, jrk0 = (np.where(seg, b[i], a[i]) for i in (2, 4, 5))
        x0d, vad, acc0d, jrk0d = (np.where(seg, tb[i], ta[i]) for i in range(4))
        vel = va + (acc0 + jrk0 * (s * 0.5)) * s
        acc = acc0 + jrk0 * s
        pd = x0d + (vad + (acc0d + jrk0d * (s * (1.0 / 3.0))) * (s * 0.5)) * s + vel * sd
        vd = vad + (acc0d + jrk0d * (s * 0.5)) * s + acc * sd
        ad = acc0d + jrk0d * s + jrk0 * sd
    return pd, vd, ad


# ---------------------------------------------------------------- inputs and measures
def scales(spline, tau=None):
    """The forward check's scales per problem, (n, 1) each: X = max|pos| + (|vel0| + |vel1| + |vel2|) T, tmin = min(duration0, duration1);
    max(X, 1) for pos, max(X / tmin, 1) for vel, max(X / tmin^2, 1) for acc."""
    p0, p1, p2, v0, v2, v1, d0, d1 = (np.abs(np.asarray(a, dtype=np.float64)) for a in spline)
    X = np.maximum(np.maximum(p0, p1), p2) + (v0 + v1 + v2) * (d0 + d1)
    tmin = np.minimum(d0, d1)
    return [np.maximum(X, 1.0)[:, None], np.maximum(X / tmin, 1.0)[:, None], np.maximum(X / tmin**2, 1.0)[:, None]]


def random_states(n, seed):
    """Random unsolved splines: positions of a few units, velocities of tens, durations 0.05 .. 2."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-5, 5, (3, n))
    v = rng.uniform(-20, 20, (3, n))
    d = rng.uniform(0.05, 2.0, (2, n))
    return [p[0], p[1], p[2], v[0], v[2], v[1], d[0], d[1]]


def query_times(spline, k, seed, exact=True, keep_off_knot=0.0):
    """tau (n, k) ~ U(-0.1, 1.1) T; with `exact` the first up to four columns of each row are 0, duration0, nextafter(duration0, 0)
    and T.  keep_off_knot: queries closer than that fraction of T to the knot are moved off it (for difference quotients)."""
    rng = np.random.default_rng(seed)
    d0, d1 = np.asarray(spline[6], dtype=np.float64), np.asarray(spline[7], dtype=np.float64)
    T = (d0 + d1)[:, None]
    tau = rng.uniform(-0.1, 1.1, (len(d0), k)) * T
    if exact:
        special = [np.zeros_like(d0), d0, np.nextafter(d0, 0.0), d0 + d1]
        for j in range(min(k, 4)):
            tau[:, j * (k // 4) if k >= 4 else j] = special[j]
    if keep_off_knot > 0.0:
        gap = tau - d0[:, None]
        near = np.abs(gap) < keep_off_knot * T
        tau = np.where(near, d0[:, None] + np.where(gap < 0, -1.0, 1.0) * keep_off_knot * T, tau)
    return np.ascontiguousarray(tau)


def normwise(a, b):
    """|a - b| / |b| per problem over everything the problem owns (arrays of n or (n, k), stacked)."""
    a = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in a], axis=1)
    b = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in b], axis=1)
    with np.errstate(all="ignore"):
        return np.asarray(np.linalg.norm((a - b).astype(np.float64), axis=1) / np.linalg.norm(b.astype(np.float64), axis=1), dtype=np.float64)
