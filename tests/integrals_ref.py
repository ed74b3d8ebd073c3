"""Test-side restatements of the integrals over time windows (rp_trajectory_integrals / _vjp / _jvp, csrc/trajectory.hip; DESIGN.md
section 16), on top of tests/trajectory_ref.py, tests/crossing_ref.py and tests/extrema_ref.py: a spline is its list of eight arrays, a
window two (n, k) arrays lo and hi (None: -inf / +inf).  The four outputs are in the entry's order, NAMES = (pos_int, distance, vel_sq,
acc_sq): the integrals of pos, |vel|, vel^2 and acc^2 over the window clamped to [0, T].

    integrals_ld     the definition in longdouble with true divisions: four (n, k) arrays, NaN where the clamped window is empty
    integrals_f64    the kernel's arithmetic in float64, operation for operation (1 / h is numpy's division where the kernel has its
                     refined reciprocal, so it restates the rule, not the bits)
    vjp_ld / jvp_ld  the derivatives with the routing of the window's ends, longdouble, plain sums
    vjp_f64 / jvp_f64
                     the same in the kernels' arithmetic, the VJP in k_trajectory_vjp's order of additions (trajectory_ref.group_lanes)
    gauss_ld         the same integrals by 3-point Gauss-Legendre on the smooth pieces through trajectory_ref.forward_ld: exact for these
                     degrees, and independent of the closed forms
    value_scales     the scales of the four outputs per unit of window length; short_windows the short-window set

Every restatement shifts to the start of the piece it integrates: (X, V, A) are pos, vel, acc at the local start sa, w the length from the
GLOBAL ends (min(b, duration0) - a or b - max(a, duration0)), and the integrals are polynomials in w with those coefficients -- no
antiderivative is differenced.  One code path serves both types: T is np.longdouble or np.float64.
"""
import numpy as np

import crossing_ref as cr
import extrema_ref as xr
import trajectory_ref as tr

LD = np.longdouble
NAMES = ("pos_int", "distance", "vel_sq", "acc_sq")


def value_scales(spline):
    """(n, 1) each: sp, sv, sv^2, sa^2 of trajectory_ref.scales -- an output's scale is this times the window's length."""
    sp, sv, sa = tr.scales(spline)
    return [sp, sv, sv * sv, sa * sa]


def clamped(spline, lo, hi, T=LD):
    """(a, b, ok) of type T, (n, k): the window clamped to [0, T] by the entry's rule (a NaN end stays NaN), and whether a <= b."""
    lo, hi = xr._window(spline, lo, hi)
    lo, hi = lo.astype(T), hi.astype(T)
    p = tr._columns(spline, np.float64)
    with np.errstate(all="ignore"):
        total = (p[6] + p[7]).astype(T)
        a = np.where(lo > 0, lo, np.where(np.isnan(lo), lo, T(0)))
        b = np.where(hi < total, hi, np.where(np.isnan(hi), hi, np.broadcast_to(total, hi.shape)))
    return a, b, a <= b


def _poly(seg, s, T):
    """pos, vel, acc of one segment at the local time s, in the evaluator's arithmetic."""
    x0, va, acc0, jrk0, _ = seg
    third, half = T(1) / T(3), T(0.5)
    return x0 + (va + (acc0 + jrk0 * (s * third)) * (s * half)) * s, va + (acc0 + jrk0 * (s * half)) * s, acc0 + jrk0 * s


def _core(spline, lo, hi, T):
    """Everything a query is made of.  Returns a dict: ok, empty (a == b), lo_taken, hi_taken, a, b, d0 and per segment a dict with
    on (the segment contributes), val[4] (its contributions), m[4][4] (the partials of each output in x0, va, acc0, jrk0), fa[4] and
    fb[4] (the integrands at the local start and end), from_a / knot_end (segment 1 starts at a / segment 0 ends on the knot)."""
    third, half, quarter = T(1) / T(3), T(0.5), T(0.25)
    segs, d0 = cr._segments(spline, T, T is LD)
    lo_w, hi_w = xr._window(spline, lo, hi)
    a, b, ok = clamped(spline, lo, hi, T)
    p = tr._columns(spline, np.float64)
    out = {"ok": ok, "a": a, "b": b, "d0": d0, "seg": []}
    with np.errstate(all="ignore"):
        total = (p[6] + p[7]).astype(T)
        out["lo_taken"] = lo_w.astype(T) > 0
        out["hi_taken"] = hi_w.astype(T) < total
        out["empty"] = ok & (a == b)
        for g, seg in enumerate(segs):
            _, va, acc0, J, h = seg
            c1, c2 = cr._breaks(va, acc0, J, h, T)
            if g == 0:
                on = ok & (a < d0)
                sa, w = a, np.where(b < d0, b, d0) - a
            else:
                on = ok & (b > d0)
                start = np.where(a > d0, a, d0)
                sa, w = start - d0, b - start
            sa, w = np.where(on, sa, T(0)), np.where(on, w, T(0))
            X, V, A = _poly(seg, sa, T)
            Xb = X + w * (V + (w * half) * (A + (w * third) * J))
            Vb = V + w * (A + (w * half) * J)
            Ab = A + w * J
            val = [None] * 4
            val[0] = w * (X + (w * half) * (V + (w * third) * (A + (w * quarter) * J)))
            val[2] = w * (V * V + w * (V * A + (w * third) * ((A * A + V * J) + w * (T(0.75) * (A * J) + ((T(3) / T(20)) * w) * (J * J)))))
            val[3] = w * (A * A + w * (A * J + (w * third) * (J * J)))
            M1 = w * (sa + w * half)
            M2 = w * (sa * sa + w * (sa + w * third))
            M3 = w * (sa * sa * sa + w * (T(1.5) * (sa * sa) + w * (sa + w * quarter)))
            Q0 = w * (V + (w * half) * (A + (w * third) * J))
            Q1 = (w * w) * (V * half + w * (A * third + (w * T(0.125)) * J))
            Q2 = (w * w * w) * (V * third + w * (A * quarter + (w * (T(1) / T(10))) * J))
            R0 = w * (A + (w * half) * J)
            R1 = (w * w) * (A * half + (w * third) * J)
            zero = T(0) * w
            m = [[w, M1, M2 * half, M3 * (T(1) / T(6))], None,
                 [zero, T(2) * Q0, T(2) * (sa * Q0 + Q1), (sa * sa) * Q0 + (T(2) * sa) * Q1 + Q2],
                 [zero, zero, T(2) * R0, T(2) * (sa * R0 + R1)]]
            # the distance: the three monotone pieces [0, c1], [c1, c2], [c2, ...) clipped to [sa, sa + w]; a piece that holds the whole
            # window has the window's own length
            se = sa + w
            dist, d1, d2, d3 = zero, zero, zero, zero
            for pl, ph in ((T(0) * c1, c1), (c1, c2), (c2, None)):
                starts = sa >= pl
                ends = (se <= ph) if ph is not None else np.ones(se.shape, dtype=bool)
                u = np.where(starts, sa, pl)
                e = np.where(ends, se, ph if ph is not None else se)
                ell = np.where(starts & ends, w, e - u)
                ell = np.where(ell > 0, ell, T(0))
                Vu, Au = va + (acc0 + J * (u * half)) * u, acc0 + J * u
                inc = ell * (Vu + (ell * half) * (Au + (ell * third) * J))
                sign = np.where(inc > 0, T(1), np.where(inc < 0, T(-1), T(0)))
                dist = dist + np.abs(inc)
                d1 = d1 + sign * ell
                d2 = d2 + sign * (ell * (u + ell * half))
                d3 = d3 + sign * (half * (ell * (u * u + ell * (u + ell * third))))
            val[1] = dist
            m[1] = [zero, d1, d2, d3]
            out["seg"].append({"on": on, "val": val, "m": m, "fa": [X, np.abs(V), V * V, A * A], "fb": [Xb, np.abs(Vb), Vb * Vb, Ab * Ab]})
        out["knot_end"] = out["seg"][0]["on"] & (b > d0)
        out["from_a"] = out["seg"][1]["on"] & (a > d0)
    return out


def _integrals(spline, lo, hi, T):
    c = _core(spline, lo, hi, T)
    with np.errstate(all="ignore"):
        return [np.where(c["ok"], np.where(c["empty"], T(0), c["seg"][0]["val"][i] + c["seg"][1]["val"][i]), T(np.nan)) for i in range(4)]


def integrals_ld(spline, lo=None, hi=None):
    """Four (n, k) longdouble arrays, NAMES' order: NaN where the clamped window is empty (or an end or the problem is NaN), +0.0 where
    a == b."""
    return _integrals(spline, lo, hi, LD)


def integrals_f64(spline, lo=None, hi=None):
    """The same in the kernel's float64 arithmetic."""
    return _integrals(spline, lo, hi, np.float64)


# ---------------------------------------------------------------- an independent quadrature
def gauss_ld(spline, lo=None, hi=None):
    """The four integrals by 3-point Gauss-Legendre in longdouble on each clamped window's smooth pieces -- split at the knot and, for the
    distance, at the velocity roots (crossing_ref.pieces_ld's seven piece ends) -- through trajectory_ref.forward_ld: exact for
    polynomials up to degree five, which is the highest here (vel^2 is of degree four)."""
    a, b, ok = clamped(spline, lo, hi, LD)
    times, _ = cr.pieces_ld(spline)                       # (n, 7): 0, c1, c2 | knot, c1, c2, T' (duration0 + duration1 in longdouble)
    d0 = np.asarray(spline[6], dtype=LD)[:, None]
    x = np.sqrt(LD(3) / LD(5))
    nodes, weights = (-x, LD(0), x), (LD(5) / 9, LD(8) / 9, LD(5) / 9)
    out = [np.zeros(a.shape, dtype=LD) for _ in range(4)]
    with np.errstate(all="ignore"):
        for j in range(6):
            # the piece clipped to the window; the last piece has no upper end of its own (the window is clamped to the float64 T), and
            # segment 0's last piece ends on duration0 itself.  Gauss nodes lie strictly inside, so each is evaluated in its own segment
            left = np.maximum(a, times[:, j:j + 1])
            right = b if j == 5 else np.minimum(b, d0 if j == 2 else times[:, j + 1:j + 2])
            live = ok & (right > left)
            length = np.where(live, right - left, LD(0))
            mid = np.where(live, left + length / 2, LD(0))
            sign = np.sign(tr.forward_ld(spline, mid)[1])
            for x_i, w_i in zip(nodes, weights):
                pos, vel, acc = tr.forward_ld(spline, mid + x_i * length / 2)
                for i, f in enumerate((pos, sign * vel, vel * vel, acc * acc)):
                    out[i] = out[i] + np.where(live, w_i * f * length / 2, LD(0))
        return [np.where(ok, o, LD(np.nan)) for o in out]


# ---------------------------------------------------------------- derivatives
def _chain(spline, S, T):
    """trajectory_ref's chain rule through (acc0, jrk0): S (8, n), the four sums of segment 0 then of segment 1 -> the eight bars without
    any end term, in the pointer table's order."""
    if T is LD:
        p0, p1, p2, v0, v2, v1, d0, d1 = [c[:, 0] for c in tr._columns(spline, LD)]
        out = []
        for which, (a0, a1, ua, ub, hh) in enumerate(((p0, p1, v0, v1, d0), (p1, p2, v1, v2, d1))):
            Sx, Sv, Sa, Sj = S[4 * which:4 * which + 4]
            a_0 = 6 * (a1 - a0) / hh**2 - (4 * ua + 2 * ub) / hh
            A = Sa - 2 / hh * Sj
            out.append((Sx - 6 * A / hh**2, 6 * A / hh**2, Sv - 4 * A / hh - 2 * Sj / hh**2, -2 * A / hh + 2 * Sj / hh**2,
                        A * (-12 * (a1 - a0) / hh**3 + (4 * ua + 2 * ub) / hh**2) + Sj * (-4 * (ub - ua) / hh**3 + 2 * a_0 / hh**2)))
    else:
        a, b, _ = tr._staged_f64(spline)
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
    return [ax0, ax1 + bx0, bx1, ava, bvb, avb + bva, ah, bh]


def _terms(spline, lo, hi, g, T):
    """Per query: the ten terms a problem's queries are summed over ((10, n, k): the four weighted partials of segment 0, of segment 1, what
    goes to duration0_bar and to duration1_bar from the window's ends), and lo_bar, hi_bar (n, k)."""
    c = _core(spline, lo, hi, T)
    ok, lo_t, hi_t = c["ok"], c["lo_taken"], c["hi_taken"]
    zero = np.zeros(ok.shape, dtype=T)
    g = [np.where(ok, np.asarray(x, dtype=T), T(0)) if x is not None else zero for x in g]
    with np.errstate(all="ignore"):
        W, Ea, Eb = [], [], []
        for s in c["seg"]:
            m = s["m"]
            W += [g[0] * m[0][0],
                  g[0] * m[0][1] + g[1] * m[1][1] + g[2] * m[2][1],
                  g[0] * m[0][2] + g[1] * m[1][2] + g[2] * m[2][2] + g[3] * m[3][2],
                  g[0] * m[0][3] + g[1] * m[1][3] + g[2] * m[2][3] + g[3] * m[3][3]]
            Ea.append(g[0] * s["fa"][0] + g[1] * s["fa"][1] + g[2] * s["fa"][2] + g[3] * s["fa"][3])
            Eb.append(g[0] * s["fb"][0] + g[1] * s["fb"][1] + g[2] * s["fb"][2] + g[3] * s["fb"][3])
        on0, on1, knot, from_a = c["seg"][0]["on"], c["seg"][1]["on"], c["knot_end"], c["from_a"]
        pick = lambda mask, x: np.where(mask, x, T(0))      # noqa: E731
        end0_b = on0 & ~knot                                 # segment 0 ends at b: hi, or (duration1 of rounding size) T
        a1 = pick(from_a & lo_t, Ea[1])
        D0 = pick(knot | (end0_b & ~hi_t), Eb[0]) + a1 - pick(on1 & hi_t, Eb[1])
        D1 = pick(on1 & ~hi_t, Eb[1]) + pick(end0_b & ~hi_t, Eb[0])
        lo_bar = -(pick(on0 & lo_t, Ea[0]) + a1)
        hi_bar = pick(end0_b & hi_t, Eb[0]) + pick(on1 & hi_t, Eb[1])
    return np.stack(W + [D0, D1], axis=0), lo_bar, hi_bar


def _finish(spline, S, T):
    bars = _chain(spline, S[:8], T)
    bars[6] = bars[6] + S[8]
    bars[7] = bars[7] + S[9]
    bad = np.isnan(tr._columns(spline, T)[6][:, 0])
    return [np.where(bad, T(np.nan), x) for x in bars]


def vjp_ld(spline, lo, hi, g):
    """(eight spline gradients (n,), lo_bar (n, k), hi_bar (n, k)) in longdouble for the upstream gradients g (four (n, k) arrays, None:
    zeros) on the four outputs; a NaN output's gradient counts as 0.  The routing of the end terms: a = lo -> lo_bar; a = +0.0 -> nowhere;
    b = hi -> hi_bar; b = T -> duration1_bar (T - duration0 is duration1: what duration0_bar gets as part of T it loses as the origin of
    segment 1's local time); segment 0's end on the knot -> duration0_bar; a segment-1 end that is lo or hi -> also duration0_bar,
    negated."""
    terms, lo_bar, hi_bar = _terms(spline, lo, hi, g, LD)
    with np.errstate(all="ignore"):
        return _finish(spline, terms.sum(axis=2), LD), lo_bar, hi_bar


def vjp_f64(spline, lo, hi, g):
    """The same as the VJP kernel forms it: float64, a problem's queries added in k_trajectory_vjp's order (G lanes from k alone, lane l
    adding units l, l + G, ..., pairs when k is even, then the xor butterfly)."""
    terms, lo_bar, hi_bar = _terms(spline, lo, hi, g, np.float64)
    _, n, k = terms.shape
    G, vec = tr.group_lanes(k)
    per = 2 if vec else 1
    units = k // per
    with np.errstate(all="ignore"):
        S = np.zeros((10, n, G))
        for first in range(0, units, G):
            lanes = np.arange(min(G, units - first))
            for e in range(per):
                S[:, :, lanes] = S[:, :, lanes] + terms[:, :, (first + lanes) * per + e]
        m = 1
        while m < G:
            S = S + S[:, :, np.arange(G) ^ m]
            m *= 2
        return _finish(spline, S[:, :, 0], np.float64), lo_bar, hi_bar


def _tangents(spline, spline_dot, T):
    """Per segment the tangents (x0d, vad, acc0d, jrk0d) as (n, 1) columns, and (duration0_dot, duration1_dot)."""
    d = [np.asarray(x, dtype=T)[:, None] if x is not None else None for x in spline_dot]
    n = len(spline[0])
    d = [x if x is not None else np.zeros((n, 1), dtype=T) for x in d]
    out = []
    with np.errstate(all="ignore"):
        if T is LD:
            p0, p1, p2, v0, v2, v1, d0, d1 = tr._columns(spline, LD)
            for x0, x1, va, vb, h, x0d, x1d, vad, vbd, hd in ((p0, p1, v0, v1, d0, d[0], d[1], d[3], d[5], d[6]),
                                                              (p1, p2, v1, v2, d1, d[1], d[2], d[5], d[4], d[7])):
                acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
                acc0d = 6 * (x1d - x0d) / h**2 - 12 * (x1 - x0) * hd / h**3 - (4 * vad + 2 * vbd) / h + (4 * va + 2 * vb) * hd / h**2
                jrk0d = 2 * (vbd - vad) / h**2 - 4 * (vb - va) * hd / h**3 - 2 * acc0d / h + 2 * acc0 * hd / h**2
                out.append((x0d, vad, acc0d, jrk0d))
        else:
            a, b, _ = tr._staged_f64(spline)
            for c, dxd, x0d, vad, vbd, hd in ((a, d[1] - d[0], d[0], d[3], d[5], d[6]), (b, d[2] - d[1], d[1], d[5], d[4], d[7])):
                x0, x1, va, vb, acc0, _, ih = c
                dx = x1 - x0
                ih2 = ih * ih
                ih3 = ih2 * ih
                acc0d = dxd * (6.0 * ih2) - dx * (12.0 * ih3) * hd - (vad * 4.0 + vbd * 2.0) * ih + (va * 4.0 + vb * 2.0) * ih2 * hd
                jrk0d = (vbd - vad) * (2.0 * ih2) - (vb - va) * (4.0 * ih3) * hd - acc0d * (2.0 * ih) + acc0 * (2.0 * ih2) * hd
                out.append((x0d, vad, acc0d, jrk0d))
    return out, d[6], d[7]


def _jvp(spline, lo, hi, spline_dot, lo_dot, hi_dot, T):
    c = _core(spline, lo, hi, T)
    ok, lo_t, hi_t = c["ok"], c["lo_taken"], c["hi_taken"]
    zero = np.zeros(ok.shape, dtype=T)
    lo_dot = np.asarray(lo_dot, dtype=T) if lo_dot is not None else zero
    hi_dot = np.asarray(hi_dot, dtype=T) if hi_dot is not None else zero
    tan, d0d, d1d = _tangents(spline, spline_dot, T)
    with np.errstate(all="ignore"):
        a_dot = np.where(lo_t, lo_dot, T(0))
        on0, on1 = c["seg"][0]["on"], c["seg"][1]["on"]
        sad = [np.where(on0, a_dot, T(0)), np.where(c["from_a"], a_dot - d0d, T(0))]
        sbd = [np.where(on0, np.where(c["knot_end"], d0d + zero, np.where(hi_t, hi_dot, d0d + d1d)), T(0)),
               np.where(on1, np.where(hi_t, hi_dot - d0d, d1d + zero), T(0))]
        out = []
        for i in range(4):
            parts = []
            for s, (x0d, vad, acc0d, jrk0d), sa_dot, sb_dot in zip(c["seg"], tan, sad, sbd):
                m = s["m"][i]
                parts.append(m[0] * x0d + m[1] * vad + m[2] * acc0d + m[3] * jrk0d + s["fb"][i] * sb_dot - s["fa"][i] * sa_dot)
            out.append(np.where(ok, parts[0] + parts[1], T(np.nan)))
    return out


def jvp_ld(spline, lo, hi, spline_dot, lo_dot, hi_dot):
    """The four output tangents (n, k) in longdouble, NaN where the output is, for tangents on the eight inputs (arrays of n, None: zeros)
    and on lo and hi ((n, k), None: zeros); the same routing as vjp_ld."""
    return _jvp(spline, lo, hi, spline_dot, lo_dot, hi_dot, LD)


def jvp_f64(spline, lo, hi, spline_dot, lo_dot, hi_dot):
    """The same as the JVP kernel forms it."""
    return _jvp(spline, lo, hi, spline_dot, lo_dot, hi_dot, np.float64)


# ---------------------------------------------------------------- inputs
def short_windows(spline, k, seed):
    """(lo, hi), (n, k): lo ~ U(0, 1) T and hi = lo + T 10^U(-9, -2) -- windows late in a segment and many orders shorter than the spline,
    where a difference of antiderivatives or of local ends would lose the window."""
    rng = np.random.default_rng(seed)
    T = (np.asarray(spline[6], dtype=np.float64) + np.asarray(spline[7], dtype=np.float64))[:, None]
    lo = rng.uniform(0.0, 1.0, (len(T), k)) * T
    hi = lo + T * 10.0 ** rng.uniform(-9.0, -2.0, (len(T), k))
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def kept_for_differences(spline, lo, hi, margin=1e-3):
    """The queries a central difference is a yardstick for, (n, k) bool: the clamped ends at least margin x T from 0, from the knot, from T
    and from each other (no end changes its class within the step); column 1, whose end sits on the knot, is left out."""
    a, b, ok = clamped(spline, lo, hi, LD)
    d0 = np.asarray(spline[6], dtype=LD)[:, None]
    T = d0 + np.asarray(spline[7], dtype=LD)[:, None]
    with np.errstate(all="ignore"):
        far = lambda x, y: np.abs(x - y) >= margin * T      # noqa: E731
        keep = ok & far(a, 0) & far(b, 0) & far(a, d0) & far(b, d0) & far(a, T) & far(b, T) & far(a, b)
    if keep.shape[1] > 1:
        keep[:, 1] = False
    return keep
