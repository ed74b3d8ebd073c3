"""Test-side restatements of the evaluator's second derivative (rp_trajectory_eval_hvp, k_trajectory_hvp in csrc/trajectory.hip; DESIGN.md
section 17): the derivative of rp_trajectory_eval_vjp's outputs (spline_bar[8], tau_bar) along a direction (spline_dot[8], tau_dot), the
upstream gradients held fixed.  Splines, tables and tau as in tests/trajectory_ref.py.

    hvp_ld       the definition in longdouble with true divisions
    hvp_f64      the kernel's own float64 arithmetic, operation for operation, and its summation order (trajectory_ref.group_lanes: G
                 lanes per problem, lane l adding its units in order, then an xor butterfly) over its eleven sums

NaN rule in both: a problem with a duration that is not finite or not > 0 is NaN everywhere.
"""
import numpy as np

import trajectory_ref as tr

LD = np.longdouble


def hvp_ld(spline, tau, gp, gv, ga, spline_dot, tau_dot):
    """(spline_bar_dot: eight arrays of n, tau_bar_dot (n, k)) in longdouble."""
    tau, gp, gv, ga, tau_dot = (np.asarray(a, dtype=LD) for a in (tau, gp, gv, ga, tau_dot))
    cols = tr._columns(spline, LD)
    dots = [np.asarray(a, dtype=LD)[:, None] for a in spline_dot]
    with np.errstate(all="ignore"):
        seg, x0, x1, va, vb, h, s = tr._select(cols, tau)
        w = lambda a, b: np.where(seg, b, a) + 0 * tau      # noqa: E731
        x0d, x1d, vad, vbd, hd = w(dots[0], dots[1]), w(dots[1], dots[2]), w(dots[3], dots[5]), w(dots[5], dots[4]), w(dots[6], dots[7])
        sd = np.where(seg, tau_dot - dots[6], tau_dot)
        acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
        jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
        acc0d = 6 * (x1d - x0d) / h**2 - 12 * (x1 - x0) * hd / h**3 - (4 * vad + 2 * vbd) / h + (4 * va + 2 * vb) * hd / h**2
        jrk0d = 2 * (vbd - vad) / h**2 - 4 * (vb - va) * hd / h**3 - 2 * acc0d / h + 2 * acc0 * hd / h**2
        acc = acc0 + jrk0 * s
        vel_d = vad + (acc0d + jrk0d * s / 2) * s + acc * sd
        acc_d = acc0d + jrk0d * s + jrk0 * sd
        tau_bar_dot = gp * vel_d + gv * acc_d + ga * jrk0d
        wt = [gp, gp * s + gv, gp * s**2 / 2 + gv * s + ga, gp * s**3 / 6 + gv * s**2 / 2 + ga * s]
        p0, p1, p2, v0, v2, v1, d0, d1 = [c[:, 0] for c in cols]
        q0, q1, q2, u0, u2, u1, e0, e1 = [d[:, 0] for d in dots]
        out = []
        for which, (a0, a1, ua, ub, hh, a0d, a1d, uad, ubd, hhd) in enumerate(((p0, p1, v0, v1, d0, q0, q1, u0, u1, e0),
                                                                              (p1, p2, v1, v2, d1, q1, q2, u1, u2, e1))):
            m = seg == bool(which)
            total = lambda x: np.sum(np.where(m, x, LD(0)), axis=1)      # noqa: E731
            Sa, Sj = total(wt[2]), total(wt[3])
            Svd, Sad, Sjd = total(wt[0] * sd), total(wt[1] * sd), total(wt[2] * sd)
            dx, dxd = a1 - a0, a1d - a0d
            a_0 = 6 * dx / hh**2 - (4 * ua + 2 * ub) / hh
            a_0d = 6 * dxd / hh**2 - 12 * dx * hhd / hh**3 - (4 * uad + 2 * ubd) / hh + (4 * ua + 2 * ub) * hhd / hh**2
            A = Sa - 2 * Sj / hh
            Ad = Sad - 2 * Sjd / hh + 2 * Sj * hhd / hh**2
            x1b = 6 * Ad / hh**2 - 12 * A * hhd / hh**3
            vab = Svd - 4 * Ad / hh + 4 * A * hhd / hh**2 - 2 * Sjd / hh**2 + 4 * Sj * hhd / hh**3
            vbb = -2 * Ad / hh + 2 * A * hhd / hh**2 + 2 * Sjd / hh**2 - 4 * Sj * hhd / hh**3
            c1 = -12 * dx / hh**3 + (4 * ua + 2 * ub) / hh**2
            c2 = -4 * (ub - ua) / hh**3 + 2 * a_0 / hh**2
            c1d = -12 * dxd / hh**3 + 36 * dx * hhd / hh**4 + (4 * uad + 2 * ubd) / hh**2 - 2 * (4 * ua + 2 * ub) * hhd / hh**3
            c2d = -4 * (ubd - uad) / hh**3 + 12 * (ub - ua) * hhd / hh**4 + 2 * a_0d / hh**2 - 4 * a_0 * hhd / hh**3
            out.append((-x1b, x1b, vab, vbb, Ad * c1 + A * c1d + Sjd * c2 + Sj * c2d))
        T1d = np.sum(np.where(seg, tau_bar_dot, LD(0)), axis=1)
        (ax0, ax1, ava, avb, ah), (bx0, bx1, bva, bvb, bh) = out
        bad = np.isnan(d0)
        bars = [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah - T1d, bh]
        bars = [np.where(bad, LD(np.nan), b) for b in bars]
    return bars, tau_bar_dot


def hvp_f64(spline, tau, gp, gv, ga, spline_dot, tau_dot):
    """(spline_bar_dot: eight arrays of n, tau_bar_dot (n, k)) float64 as k_trajectory_hvp forms them, in its order of additions."""
    tau, gp, gv, ga, tau_dot = (np.asarray(x, dtype=np.float64) for x in (tau, gp, gv, ga, tau_dot))
    n, k = tau.shape
    a, b, d0 = tr._staged_f64(spline)
    d = [np.asarray(x, dtype=np.float64)[:, None] for x in spline_dot]

    def tangents(c, dxd, vad, vbd, hd):      # segment_tangents
        x0, x1, va, vb, acc0, _, ih = c
        dx = x1 - x0
        ih2 = ih * ih
        ih3 = ih2 * ih
        acc0d = dxd * (6.0 * ih2) - dx * (12.0 * ih3) * hd - (vad * 4.0 + vbd * 2.0) * ih + (va * 4.0 + vb * 2.0) * ih2 * hd
        jrk0d = (vbd - vad) * (2.0 * ih2) - (vb - va) * (4.0 * ih3) * hd - acc0d * (2.0 * ih) + acc0 * (2.0 * ih2) * hd
        return acc0d, jrk0d

    with np.errstate(all="ignore"):
        # per segment along the direction: vad, vbd, dxd, hd, acc0d, jrk0d
        ta = (d[3], d[5], d[1] - d[0], d[6]) + tangents(a, d[1] - d[0], d[3], d[5], d[6])
        tb = (d[5], d[4], d[2] - d[1], d[7]) + tangents(b, d[2] - d[1], d[5], d[4], d[7])
        seg = ~(tau < d0)
        s = np.where(seg, tau - d0, tau)
        sd = np.where(seg, tau_dot - d[6], tau_dot)
        acc0, jrk0 = (np.where(seg, b[i], a[i]) for i in (4, 5))
        vad, acc0d, jrk0d = (np.where(seg, tb[i], ta[i]) for i in (0, 4, 5))
        acc = acc0 + jrk0 * s
        vel_d = vad + (acc0d + jrk0d * (s * 0.5)) * s + acc * sd
        acc_d = acc0d + jrk0d * s + jrk0 * sd
        tbd = gp * vel_d + gv * acc_d + ga * jrk0d
        h2 = s * (s * 0.5)
        h3 = h2 * (s * (1.0 / 3.0))
        w0, w1, w2, w3 = gp, gp * s + gv, gp * h2 + gv * s + ga, gp * h3 + gv * h2 + ga * s
        per_seg = [w2, w3, w0 * sd, w1 * sd, w2 * sd]
        terms = [np.where(seg, 0.0, x) for x in per_seg] + [np.where(seg, x, 0.0) for x in per_seg] + [np.where(seg, tbd, 0.0)]
        terms = np.stack(terms, axis=0)                      # (11, n, k)
        G, vec = tr.group_lanes(k)
        per = 2 if vec else 1
        units = k // per
        S = np.zeros((11, n, G))
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
        for which, (c, t) in enumerate(((a, ta), (b, tb))):
            xa, xb, va, vb, acc0, _, ih = (x[:, 0] for x in c)
            vad, vbd, dxd, hd, acc0d, _ = (x[:, 0] for x in t)
            Sa, Sj, Svd, Sad, Sjd = S[5 * which:5 * which + 5]
            dx = xb - xa
            ih2 = ih * ih
            ih3 = ih2 * ih
            ih4 = ih2 * ih2
            A = Sa - (2.0 * ih) * Sj
            Ad = Sad - (2.0 * ih) * Sjd + ((2.0 * ih2) * Sj) * hd
            x1b = (6.0 * ih2) * Ad - ((12.0 * ih3) * A) * hd
            vab = Svd - (4.0 * ih) * Ad + ((4.0 * ih2) * A) * hd - (2.0 * ih2) * Sjd + ((4.0 * ih3) * Sj) * hd
            vbb = (2.0 * ih2) * Sjd - (2.0 * ih) * Ad + ((2.0 * ih2) * A) * hd - ((4.0 * ih3) * Sj) * hd
            c1 = (va * 4.0 + vb * 2.0) * ih2 - dx * (12.0 * ih3)
            c2 = acc0 * (2.0 * ih2) - (vb - va) * (4.0 * ih3)
            c1d = (vad * 4.0 + vbd * 2.0) * ih2 - dxd * (12.0 * ih3) + (dx * (36.0 * ih4) - (va * 4.0 + vb * 2.0) * (2.0 * ih3)) * hd
            c2d = acc0d * (2.0 * ih2) - (vbd - vad) * (4.0 * ih3) + ((vb - va) * (12.0 * ih4) - acc0 * (4.0 * ih3)) * hd
            out.append((-x1b, x1b, vab, vbb, Ad * c1 + A * c1d + Sjd * c2 + Sj * c2d))
        (ax0, ax1, ava, avb, ah), (bx0, bx1, bva, bvb, bh) = out
        bars = [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah - S[10], bh]
    return bars, tbd


def directions(n, k, seed):
    """A random direction: (eight arrays of n, (n, k))."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(8)], rng.standard_normal((n, k))


def gradients(n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, k)) for _ in range(3)]


def translation(n):
    """pos0_dot = pos1_dot = pos2_dot = 1, everything else 0: the spline moves as a whole, no derivative of it changes."""
    one, zero = np.ones(n), np.zeros(n)
    return [one, one, one, zero, zero, zero, zero, zero]


def bilinear(bars_dot, tau_bar_dot, dots, tdot):
    """u^T (H v) for H v = (bars_dot, tau_bar_dot) and u = (dots, tdot), per problem in longdouble: (the value, the sum of |terms|)."""
    terms = [np.asarray(b, dtype=LD) * np.asarray(x, dtype=LD) for b, x in zip(bars_dot, dots)]
    per_query = np.asarray(tau_bar_dot, dtype=LD) * np.asarray(tdot, dtype=LD)
    return sum(terms) + np.sum(per_query, axis=1), sum(np.abs(t) for t in terms) + np.sum(np.abs(per_query), axis=1)
