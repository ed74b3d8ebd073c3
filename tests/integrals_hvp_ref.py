"""Test-side restatements of the integrals' second derivative (rp_trajectory_integrals_hvp, k_window_hvp in csrc/trajectory.hip; DESIGN.md
section 19), on top of tests/integrals_ref.py: the derivative of rp_trajectory_integrals_vjp's ten outputs (spline_bar[8], lo_bar, hi_bar)
along a direction (spline_dot[8], lo_dot, hi_dot), the upstream gradients g held fixed and everything that routes (lo_taken, hi_taken,
which segment contributes, where segment 0 ends) as the forward took it.

    hvp_ld       the definition in longdouble with true divisions, plain sums, section 16's routing
    hvp_f64      the kernel's own float64 arithmetic, operation for operation, and its order of additions (trajectory_ref.group_lanes: G
                 lanes per problem, lane l adding its units in order, then an xor butterfly) over its fourteen sums

One code path serves both types, as in integrals_ref.  Per segment and query, with C = (x0, va, acc0, jrk0), the direction C_dot on them
(integrals_ref._tangents), sad and sbd on the piece's local ends, phi = (0, 1, s, s^2 / 2) and Nm the integral of s^m over the piece:

    (dI / dC)_dot = (d2I / dC2) C_dot + (df(sb) / dC) sbd - (df(sa) / dC) sad
    f(end)_dot    = (df(end) / dC) C_dot + f'(end) end_dot
    distance      a breakpoint c that is a root (c1 != 0, c2 != h) with sa < c < sa + w adds 2 vel_dot(c) / |acc(c)| (1, c, c^2 / 2) to the
                  dotted partials in (va, acc0, jrk0); acc(c) == 0 adds nothing

NaN rule in both: a problem with a duration that is not finite or not > 0 is NaN in its eight results; a query whose outputs are NaN counts
with g = 0 and has lo_bar_dot = hi_bar_dot = 0.
"""
import numpy as np

import crossing_ref as cr
import integrals_ref as ir
import trajectory_ref as tr

LD = np.longdouble
SUMS = 14


def _dense(x, shape, T):
    return np.zeros(shape, dtype=T) if x is None else np.asarray(x, dtype=T)


def _terms(spline, lo, hi, g, spline_dot, lo_dot, hi_dot, T):
    """Per query the fourteen terms a problem's queries are summed over ((14, n, k): per segment the first-order weighted partials in acc0
    and jrk0, then the dotted ones in x0, va, acc0, jrk0; then what the window's ends put on duration0_bar_dot and duration1_bar_dot), and
    lo_bar_dot, hi_bar_dot (n, k)."""
    third, half = T(1) / T(3), T(0.5)
    c = ir._core(spline, lo, hi, T)
    ok, lo_t, hi_t, a, b, d0 = c["ok"], c["lo_taken"], c["hi_taken"], c["a"], c["b"], c["d0"]
    shape = ok.shape
    g = [np.where(ok, _dense(x, shape, T), T(0)) for x in (g if g is not None else [None] * 4)]
    lo_dot, hi_dot = _dense(lo_dot, shape, T), _dense(hi_dot, shape, T)
    segs, _ = cr._segments(spline, T, T is LD)
    tan, d0d, d1d = ir._tangents(spline, spline_dot if spline_dot is not None else [None] * 8, T)
    zero = np.zeros(shape, dtype=T)
    pick = lambda mask, x: np.where(mask, x, T(0))      # noqa: E731
    sign = lambda x: np.where(x > 0, T(1), np.where(x < 0, T(-1), T(0)))      # noqa: E731
    vel_at = lambda va_, acc_, jrk_, s: va_ + (acc_ + jrk_ * (s * half)) * s      # noqa: E731
    pos_at = lambda x_, va_, acc_, jrk_, s: x_ + (va_ + (acc_ + jrk_ * (s * third)) * (s * half)) * s      # noqa: E731
    with np.errstate(all="ignore"):
        a_dot = np.where(lo_t, lo_dot, T(0))
        on0, on1, knot, from_a = c["seg"][0]["on"], c["seg"][1]["on"], c["knot_end"], c["from_a"]
        sads = [pick(on0, a_dot), pick(from_a, a_dot - d0d)]
        sbds = [pick(on0, np.where(b > d0, d0d + zero, np.where(hi_t, hi_dot, d0d + d1d))), pick(on1, np.where(hi_t, hi_dot - d0d, d1d + zero))]
        terms, Ea, Eb = [], [], []
        for which, (seg, core, (x0d, vad, acc0d, jrk0d), sad, sbd) in enumerate(zip(segs, c["seg"], tan, sads, sbds)):
            _, va, acc0, J, h = seg
            on = core["on"]
            if which == 0:
                sa, w = a, np.where(b < d0, b, d0) - a
            else:
                start = np.where(a > d0, a, d0)
                sa, w = start - d0, b - start
            sa, w = np.where(on, sa, T(0)), np.where(on, w, T(0))
            sb = sa + w
            X, V, A = ir._poly(seg, sa, T)
            Vb, Ab = V + w * (A + (w * half) * J), A + w * J
            vda, vdb = vel_at(vad, acc0d, jrk0d, sa), vel_at(vad, acc0d, jrk0d, sb)
            ada, adb = acc0d + jrk0d * sa, acc0d + jrk0d * sb
            Va_dot, Vb_dot = vda + A * sad, vdb + Ab * sbd
            ha, hb = sa * (sa * half), sb * (sb * half)
            ta, tb = ha * (sa * third), hb * (sb * third)
            n, fad, fbd = [None] * 4, [None] * 4, [None] * 4
            n[0] = [sbd - sad, sb * sbd - sa * sad, hb * sbd - ha * sad, tb * sbd - ta * sad]
            fad[0], fbd[0] = pos_at(x0d, vad, acc0d, jrk0d, sa) + V * sad, pos_at(x0d, vad, acc0d, jrk0d, sb) + Vb * sbd
            # the distance: the ends, and the roots strictly inside the piece
            c1, c2 = cr._breaks(va, acc0, J, h, T)
            root1, root2 = c1 != 0, c2 != h
            factor = []
            for cc, root in ((c1, root1), (c2, root2)):
                acc_c = acc0 + J * cc
                live = root & (acc_c != 0)
                f = np.where(live, T(2) * vel_at(vad, acc0d, jrk0d, cc) / np.where(live, np.abs(acc_c), T(1)), T(0))
                factor.append(np.where(np.isfinite(f), f, T(0)))
            # the sign of the velocity just inside each end: the segment's first sign -- that at the middle of the longest of the three
            # pieces, turned back by the roots before it -- turned once per root passed (a root on the start is passed, one on the end not)
            l0, l1, l2 = c1, c2 - c1, h - c2
            piece = np.where((l0 >= l1) & (l0 >= l2), 0, np.where(l1 >= l2, 1, 2))
            mid = np.where(piece == 0, half * c1, np.where(piece == 1, c1 + half * l1, c2 + half * l2))
            s0 = sign(vel_at(va, acc0, J, mid))
            s0 = np.where(((piece >= 1) & root1) != ((piece == 2) & root2), -s0, s0)
            odd_a = (root1 & (c1 <= sa)) != (root2 & (c2 <= sa))
            odd_b = (root1 & (c1 < sb)) != (root2 & (c2 < sb))
            ga, gb = np.where(odd_a, -s0, s0 + zero), np.where(odd_b, -s0, s0 + zero)
            ea, eb = ga * sad, gb * sbd
            r1, r2 = pick(root1 & (c1 > sa) & (c1 < sb), factor[0] + zero), pick(root2 & (c2 > sa) & (c2 < sb), factor[1] + zero)
            n[1] = [zero, (eb - ea) + (r1 + r2), (sb * eb - sa * ea) + (c1 * r1 + c2 * r2),
                    (hb * eb - ha * ea) + ((c1 * (c1 * half)) * r1 + (c2 * (c2 * half)) * r2)]
            fad[1], fbd[1] = ga * Va_dot, gb * Vb_dot
            # vel_sq and acc_sq: the moments of s over the piece, from its start and its length
            N1, N2 = w * (sa + w * half), w * (sa * sa + w * (sa + w * third))
            s2 = sa * sa
            N3 = w * (s2 * sa + w * (T(1.5) * s2 + w * (sa + w * T(0.25))))
            N4 = w * (s2 * s2 + w * (T(2) * (s2 * sa) + w * (T(2) * s2 + w * (sa + w * (T(1) / T(5))))))
            hj = half * jrk0d
            ea, eb = (T(2) * V) * sad, (T(2) * Vb) * sbd
            n[2] = [zero, T(2) * (w * vad + N1 * acc0d + N2 * hj) + (eb - ea), T(2) * (N1 * vad + N2 * acc0d + N3 * hj) + (sb * eb - sa * ea),
                    (N2 * vad + N3 * acc0d + N4 * hj) + (hb * eb - ha * ea)]
            fad[2], fbd[2] = (T(2) * V) * Va_dot, (T(2) * Vb) * Vb_dot
            ea, eb = (T(2) * A) * sad, (T(2) * Ab) * sbd
            n[3] = [zero, zero, T(2) * (w * acc0d + N1 * jrk0d) + (eb - ea), T(2) * (N1 * acc0d + N2 * jrk0d) + (sb * eb - sa * ea)]
            fad[3], fbd[3] = (T(2) * A) * (ada + J * sad), (T(2) * Ab) * (adb + J * sbd)
            m = core["m"]
            terms += [g[0] * m[0][2] + g[1] * m[1][2] + g[2] * m[2][2] + g[3] * m[3][2],
                      g[0] * m[0][3] + g[1] * m[1][3] + g[2] * m[2][3] + g[3] * m[3][3],
                      g[0] * n[0][0],
                      g[0] * n[0][1] + g[1] * n[1][1] + g[2] * n[2][1],
                      g[0] * n[0][2] + g[1] * n[1][2] + g[2] * n[2][2] + g[3] * n[3][2],
                      g[0] * n[0][3] + g[1] * n[1][3] + g[2] * n[2][3] + g[3] * n[3][3]]
            Ea.append(g[0] * fad[0] + g[1] * fad[1] + g[2] * fad[2] + g[3] * fad[3])
            Eb.append(g[0] * fbd[0] + g[1] * fbd[1] + g[2] * fbd[2] + g[3] * fbd[3])
        end0_b = on0 & ~knot
        a1 = pick(from_a & lo_t, Ea[1])
        D0 = pick(knot | (end0_b & ~hi_t), Eb[0]) + a1 - pick(on1 & hi_t, Eb[1])
        D1 = pick(on1 & ~hi_t, Eb[1]) + pick(end0_b & ~hi_t, Eb[0])
        lo_bar_dot = -(pick(on0 & lo_t, Ea[0]) + a1)
        hi_bar_dot = pick(end0_b & hi_t, Eb[0]) + pick(on1 & hi_t, Eb[1])
    return np.stack([t + zero for t in terms] + [D0, D1], axis=0), lo_bar_dot, hi_bar_dot


def _finish(spline, spline_dot, S, T):
    """The fourteen sums (14, n) -> the eight results: segment_chain_dot per segment, S_xd beside its x0, the end terms on the durations."""
    n = len(spline[0])
    d = [np.zeros(n, dtype=T) if x is None else np.asarray(x, dtype=T) for x in (spline_dot if spline_dot is not None else [None] * 8)]
    out = []
    with np.errstate(all="ignore"):
        if T is LD:
            p0, p1, p2, v0, v2, v1, d0, d1 = [c[:, 0] for c in tr._columns(spline, LD)]
            for which, (a0, a1, ua, ub, hh, a0d, a1d, uad, ubd, hhd) in enumerate(((p0, p1, v0, v1, d0, d[0], d[1], d[3], d[5], d[6]),
                                                                                  (p1, p2, v1, v2, d1, d[1], d[2], d[5], d[4], d[7]))):
                Sa, Sj, Sxd, Svd, Sad, Sjd = S[6 * which:6 * which + 6]
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
                out.append((-x1b + Sxd, x1b, vab, vbb, Ad * c1 + A * c1d + Sjd * c2 + Sj * c2d))
        else:
            sa_, sb_, _ = tr._staged_f64(spline)
            tan, _, _ = ir._tangents(spline, d, np.float64)
            for which, (c, t, vbd, dxd, hd) in enumerate(((sa_, tan[0], d[5], d[1] - d[0], d[6]), (sb_, tan[1], d[4], d[2] - d[1], d[7]))):
                xa, xb, va, vb, acc0, _, ih = (x[:, 0] for x in c)
                vad, acc0d = t[1][:, 0], t[2][:, 0]
                Sa, Sj, Sxd, Svd, Sad, Sjd = S[6 * which:6 * which + 6]
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
                out.append((-x1b + Sxd, x1b, vab, vbb, Ad * c1 + A * c1d + Sjd * c2 + Sj * c2d))
        (ax0, ax1, ava, avb, ah), (bx0, bx1, bva, bvb, bh) = out
        bars = [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah + S[12], bh + S[13]]
        bad = np.isnan(tr._columns(spline, T)[6][:, 0])
        return [np.where(bad, T(np.nan), x) for x in bars]


def hvp_ld(spline, lo, hi, g, spline_dot, lo_dot, hi_dot):
    """(spline_bar_dot: eight arrays of n, lo_bar_dot (n, k), hi_bar_dot (n, k)) in longdouble; g four (n, k) arrays, spline_dot eight arrays
    of n, lo_dot and hi_dot (n, k) -- None anywhere: zeros."""
    terms, lo_bar_dot, hi_bar_dot = _terms(spline, lo, hi, g, spline_dot, lo_dot, hi_dot, LD)
    with np.errstate(all="ignore"):
        return _finish(spline, spline_dot, terms.sum(axis=2), LD), lo_bar_dot, hi_bar_dot


def hvp_f64(spline, lo, hi, g, spline_dot, lo_dot, hi_dot):
    """The same as k_window_hvp forms it: float64, a problem's queries added in k_trajectory_vjp's order."""
    terms, lo_bar_dot, hi_bar_dot = _terms(spline, lo, hi, g, spline_dot, lo_dot, hi_dot, np.float64)
    _, n, k = terms.shape
    G, vec = tr.group_lanes(k)
    per = 2 if vec else 1
    units = k // per
    with np.errstate(all="ignore"):
        S = np.zeros((SUMS, n, G))
        for first in range(0, units, G):
            lanes = np.arange(min(G, units - first))
            for e in range(per):
                S[:, :, lanes] = S[:, :, lanes] + terms[:, :, (first + lanes) * per + e]
        m = 1
        while m < G:
            S = S + S[:, :, np.arange(G) ^ m]
            m *= 2
        return _finish(spline, spline_dot, S[:, :, 0], np.float64), lo_bar_dot, hi_bar_dot


# ---------------------------------------------------------------- inputs and measures
def directions(spline, lo, seed, scaled=None):
    """A random direction in all ten inputs: (eight arrays of n, lo_dot (n, k), hi_dot (n, k)).  With `scaled` = (lo, hi) every component
    is multiplied by max(|x|, 1) of its input, so that a step e along it moves each input by e max(|x|, 1) times a standard normal."""
    rng = np.random.default_rng(seed)
    n = len(spline[0])
    dots = [rng.standard_normal(n) for _ in range(8)]
    lo_dot, hi_dot = rng.standard_normal(np.shape(lo)), rng.standard_normal(np.shape(lo))
    if scaled is not None:
        size = lambda x: np.maximum(np.abs(np.where(np.isfinite(x), x, 0.0)), 1.0)      # noqa: E731
        dots = [d * size(np.asarray(x, dtype=np.float64)) for d, x in zip(dots, spline)]
        lo_dot, hi_dot = lo_dot * size(scaled[0]), hi_dot * size(scaled[1])
    return dots, lo_dot, hi_dot


def gradients(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape) for _ in range(4)]


def translation(n):
    """pos0_dot = pos1_dot = pos2_dot = 1, everything else 0: the spline moves as a whole."""
    one, zero = np.ones(n), np.zeros(n)
    return [one, one, one, zero, zero, zero, zero, zero]


def bilinear(result, direction):
    """u^T (H v) for H v = result = (bars_dot, lo_bar_dot, hi_bar_dot) and u = direction = (dots, lo_dot, hi_dot), per problem in longdouble:
    (the value, the sum of |terms|)."""
    bars, lb, hb = result
    dots, ld, hd = direction
    terms = [np.asarray(x, dtype=LD) * np.asarray(y, dtype=LD) for x, y in zip(bars, dots)]
    per_query = np.asarray(lb, dtype=LD) * np.asarray(ld, dtype=LD) + np.asarray(hb, dtype=LD) * np.asarray(hd, dtype=LD)
    sizes = np.abs(np.asarray(lb, dtype=LD) * np.asarray(ld, dtype=LD)) + np.abs(np.asarray(hb, dtype=LD) * np.asarray(hd, dtype=LD))
    return sum(terms) + per_query.sum(axis=1), sum(np.abs(t) for t in terms) + sizes.sum(axis=1)


def flat(result):
    """(bars, lo_bar_dot, hi_bar_dot) as one list of ten arrays, for trajectory_ref.normwise."""
    return list(result[0]) + [result[1], result[2]]


def kept_for_hvp_differences(spline, lo, hi):
    """integrals_ref.kept_for_differences less the queries where a central difference of the first-order rule is no yardstick for the root
    term: a velocity root within 1e-3 T of a clamped window end (the step moves it across), and a root inside the window where
    |acc(root)| < 1e-2 (|acc0| + |jrk0| h) (a near-double root: the term is large and the difference's truncation with it).  Returns
    (kept, whether a root lies strictly inside the window), (n, k) bool each."""
    keep = ir.kept_for_differences(spline, lo, hi)
    a, b, ok = ir.clamped(spline, lo, hi, LD)
    segs, d0 = cr._segments(spline, LD, True)
    total = d0 + np.asarray(spline[7], dtype=LD)[:, None]
    inside = np.zeros(keep.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for which, (_, va, acc0, J, h) in enumerate(segs):
            c1, c2 = cr._breaks(va, acc0, J, h, LD)
            for cc, root in ((c1, c1 != 0), (c2, c2 != h)):
                t = cc + (d0 if which else 0)
                near = root & ((np.abs(t - a) < 1e-3 * total) | (np.abs(t - b) < 1e-3 * total))
                within = root & ok & (t > a) & (t < b)
                flat_root = within & (np.abs(acc0 + J * cc) < 1e-2 * (np.abs(acc0) + np.abs(J) * h))
                keep &= ~(near | flat_root)
                inside |= within
    return keep, inside



def keeps_the_end_velocities(dots):
    """The direction with vel0_dot = vel2_dot = 0: tangent to the set of rest-to-rest splines.  Where an end velocity is zero the root of
    the velocity sits on the spline's own end, and along a direction that moves that velocity the root enters the window for one sign of
    the step only: the distance's second derivative is one-sided there, and which side the comparison sa < c < sa + w gives is decided by
    rounding.  Along a direction that keeps it the root stays on the end and the derivative is two-sided: the comparisons between
    precisions on the rest-to-rest families go along such directions."""
    dots = list(dots)
    dots[3], dots[4] = np.zeros_like(dots[3]), np.zeros_like(dots[4])
    return dots
