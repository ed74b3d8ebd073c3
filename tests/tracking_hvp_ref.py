"""Test-side restatements of the tracking integrals' second derivative (rp_trajectory_tracking_hvp, k_pair_hvp in csrc/trajectory.hip;
DESIGN.md section 23), on top of tests/tracking_ref.py: the derivative of rp_trajectory_tracking_vjp's nineteen outputs (A's eight bars,
B's eight, lo_bar, hi_bar, delay_bar) along a direction (a_dot[8], b_dot[8], lo_dot, hi_dot, delay_dot), the upstream gradients g held
fixed and everything that routes (the classes of a and b, the order of the knots, which knot is clamped to which end, the segment each
spline is in on a piece) as the forward took it.

    hvp_ld       the definition in longdouble with true divisions, plain sums, section 20's routing
    hvp_f64      the kernel's float64 arithmetic and its order of additions (trajectory_ref.group_lanes: G lanes per problem, lane l adding
                 its units in order, then an xor butterfly) over its fourteen sums per side (1 / h is numpy's division where the kernel has
                 its refined reciprocal, so it restates the rule, not the bits)

One code path serves both types.  Per piece, with (Xd, Vd, Ad, Jd) the tangent of the piece's state at fixed u, wd = ed - cd, and the
moments Em, Qm linear in the state:

    Em_dot = Em(Xd, Vd, Ad, Jd) + D(w) w^m wd        Qm_dot = Qm(Vd, Ad, Jd) + D'(w) w^m wd
    (Xb, Vb, Ab, Jb)_dot term by term; W[f]_dot = W[f](dotted) + W[f - 1] sd; P_A_dot, P_B_dot by the product rule
    F_dot = (g0 + 2 g1 D(w)) (D_d(w) + D'(w) wd) + 2 g2 D'(w) (D'_d(w) + D''(w) wd)

NaN rule in both: a problem either of whose splines has a duration that is not finite or not > 0 is NaN in its sixteen per-problem results;
a query whose outputs are NaN counts with g = 0 and with query tangents of 0 and has lo_bar_dot = hi_bar_dot = delay_bar_dot = 0.
"""
import numpy as np

import integrals_hvp_ref as ih
import tracking_ref as tk
import trajectory_ref as tr

LD = np.longdouble
SUMS = 14


def _dense(x, shape, T):
    return np.zeros(shape, dtype=T) if x is None else np.asarray(x, dtype=T)


def _end_gap(t, w, T):
    return t["X"] + w * (t["V"] + (w * T(0.5)) * (t["A"] + (w * (T(1) / T(3))) * t["J"]))


def _end_rate(t, w, T):
    return t["V"] + w * (t["A"] + (w * T(0.5)) * t["J"])


def _gap_moments(t, w, T):
    X, V, A, J, w2 = t["X"], t["V"], t["A"], t["J"], w * w
    c = lambda p, q: T(p) / T(q)      # noqa: E731
    return [w * (X + w * (V * T(0.5) + w * (A * c(1, 6) + (w * c(1, 24)) * J))),
            w2 * (X * T(0.5) + w * (V * c(1, 3) + w * (A * T(0.125) + (w * c(1, 30)) * J))),
            (w2 * w) * (X * c(1, 3) + w * (V * T(0.25) + w * (A * c(1, 10) + (w * c(1, 36)) * J))),
            (w2 * w2) * (X * T(0.25) + w * (V * c(1, 5) + w * (A * c(1, 12) + (w * c(1, 42)) * J)))]


def _rate_moments(t, w, T):
    V, A, J = t["V"], t["A"], t["J"]
    c = lambda p, q: T(p) / T(q)      # noqa: E731
    return [w * (V + (w * T(0.5)) * (A + (w * c(1, 3)) * J)), (w * w) * (V * T(0.5) + w * (A * c(1, 3) + (w * T(0.125)) * J)),
            (w * w * w) * (V * c(1, 3) + w * (A * T(0.25) + (w * c(1, 10)) * J))]


def _terms(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, delay_dot, T):
    """Per query the fourteen terms a problem's queries are summed over, for each side ((14, n, k) each: per segment the reverse rule's
    weights on acc0 and jrk0, then the dotted ones on x0, va, acc0, jrk0; then what the piece ends put on duration0_bar_dot and
    duration1_bar_dot), and lo_bar_dot, hi_bar_dot, delay_bar_dot (n, k)."""
    walk = tk._walk(a, b, lo, hi, delay, T)
    ca, cb = tk._constants(a, T), tk._constants(b, T)
    ok = walk["ok"]
    shape = ok.shape
    zero = np.zeros(shape, dtype=T)
    col = lambda x: np.zeros((shape[0], 1), dtype=T) if x is None else np.asarray(x, dtype=T)[:, None]      # noqa: E731
    da, db = [col(x) for x in (a_dot or [None] * 8)], [col(x) for x in (b_dot or [None] * 8)]
    g = [np.where(ok, _dense(x, shape, T), T(0)) for x in (g if g is not None else [None] * 3)]
    lod, hid, dld = (np.where(ok, _dense(x, shape, T), T(0)) for x in (lo_dot, hi_dot, delay_dot))
    live = lambda x: np.where(ok, x, T(0))      # noqa: E731
    third, half = T(1) / T(3), T(0.5)
    with np.errstate(all="ignore"):
        tan = {}
        for side, c, d in (("a", ca, da), ("b", cb, db)):
            both = [tk._tangents(c[0], d[1] - d[0], d[0], d[3], d[5], d[6]), tk._tangents(c[1], d[2] - d[1], d[1], d[5], d[4], d[7])]
            tan[side] = [{"x0": t[0], "va": t[1], "acc0": t[2], "jrk0": t[3]} for t in both]
        ad = np.where(walk["cls_a"] == tk.A_LO, lod, np.where(walk["cls_a"] == tk.A_START, dld, T(0)))
        bd = np.where(walk["cls_b"] == tk.B_HI, hid, np.where(walk["cls_b"] == tk.B_END_A, da[6] + da[7], dld + (db[6] + db[7])))
        kAd, kBd = da[6] + zero, dld + db[6]
        tangent = lambda kind: np.where(kind == tk.END_A, ad, np.where(kind == tk.END_B, bd, np.where(kind == tk.KNOT_A, kAd, kBd)))      # noqa: E731
        sums = {side: [zero] * SUMS for side in "ab"}
        # per side, k_pair_hvp's accumulators: what a and b take, the own duration0 (its knot as a piece end and as an offset), the delay
        bar_a, bar_b, dl, carry = zero, zero, zero, zero
        own0 = {"a": zero, "b": zero}
        pick = lambda mask, v: np.where(mask, v, T(0))      # noqa: E731
        for p in walk["pieces"]:
            t = tk._state(ca, cb, p, T)
            w = p["w"]
            cd, ed = tangent(p["kind_c"]), tangent(p["kind_e"])
            dsA = cd - np.where(p["seg_a"], kAd, T(0))
            dsB = cd - np.where(p["seg_b"], kBd, dld)
            wd = ed - cd
            XAd, VAd, AAd, JAd = tk._local(tan["a"], p["seg_a"], p["sA"], T)
            XBd, VBd, ABd, JBd = tk._local(tan["b"], p["seg_b"], p["sB"], T)
            XAd, VAd, AAd = XAd + t["VA"] * dsA, VAd + t["AA"] * dsA, AAd + t["JA"] * dsA
            XBd, VBd, ABd = XBd + t["VB"] * dsB, VBd + t["AB"] * dsB, ABd + t["JB"] * dsB
            td = {"X": XAd - XBd, "V": VAd - VBd, "A": AAd - ABd, "J": JAd - JBd}
            w2 = w * (w * half)
            w3 = w2 * (w * third)
            Dw, Vw, Aw = _end_gap(t, w, T), _end_rate(t, w, T), t["A"] + w * t["J"]
            Ddw, Vdw = _end_gap(td, w, T), _end_rate(td, w, T)
            Xb, Vb, Ab, Jb = g[0] * w, g[0] * w2, g[0] * w3, g[0] * (w3 * (w * T(0.25)))
            Xbd, Vbd, Abd, Jbd = g[0] * wd, g[0] * (w * wd), g[0] * (w2 * wd), g[0] * (w3 * wd)
            E, Ed = _gap_moments(t, w, T), _gap_moments(td, w, T)
            h, e = T(2) * g[1], Dw * wd
            Ed = [Ed[0] + e, Ed[1] + w * e, Ed[2] + (w * w) * e, Ed[3] + (w * w * w) * e]
            Xb, Vb, Ab, Jb = Xb + h * E[0], Vb + h * E[1], Ab + g[1] * E[2], Jb + g[1] * (E[3] * third)
            Xbd, Vbd, Abd, Jbd = Xbd + h * Ed[0], Vbd + h * Ed[1], Abd + g[1] * Ed[2], Jbd + g[1] * (Ed[3] * third)
            Q, Qd = _rate_moments(t, w, T), _rate_moments(td, w, T)
            h, e = T(2) * g[2], Vw * wd
            Qd = [Qd[0] + e, Qd[1] + w * e, Qd[2] + (w * w) * e]
            Vb, Ab, Jb = Vb + h * Q[0], Ab + h * Q[1], Jb + g[2] * Q[2]
            Vbd, Abd, Jbd = Vbd + h * Qd[0], Abd + h * Qd[1], Jbd + g[2] * Qd[2]
            for side, s, sd, seg, sign in (("a", p["sA"], dsA, p["seg_a"], 1), ("b", p["sB"], dsB, p["seg_b"], -1)):
                h2 = s * (s * half)
                h3 = h2 * (s * third)
                W1, W2, W3 = Xb * s + Vb, Xb * h2 + Vb * s + Ab, Xb * h3 + Vb * h2 + Ab * s + Jb
                U = [W2, W3, Xbd + zero, (Xbd * s + Vbd) + Xb * sd, (Xbd * h2 + Vbd * s + Abd) + W1 * sd,
                     (Xbd * h3 + Vbd * h2 + Abd * s + Jbd) + W2 * sd]
                new = list(sums[side])
                for f in range(6):
                    Uf = live(sign * U[f])
                    new[f] = new[f] + np.where(seg, T(0), Uf)
                    new[6 + f] = new[6 + f] + np.where(seg, Uf, T(0))
                sums[side] = new
            Fd = live((g[0] + (T(2) * g[1]) * Dw) * (Ddw + Vw * wd) + ((T(2) * g[2]) * Vw) * (Vdw + Aw * wd))
            PAd = live((Xbd * t["VA"] + Vbd * t["AA"] + Abd * t["JA"]) + (Xb * VAd + Vb * AAd + Ab * JAd))
            PBd = live((Xbd * t["VB"] + Vbd * t["AB"] + Abd * t["JB"]) + (Xb * VBd + Vb * ABd + Ab * JBd))
            v = carry + ((PAd - PBd) - Fd)
            kind = p["kind_c"]
            bar_a, bar_b = bar_a + pick(kind == tk.END_A, v), bar_b + pick(kind == tk.END_B, v)
            own0["a"] = own0["a"] + pick(kind == tk.KNOT_A, v)
            own0["b"] = own0["b"] + pick(kind == tk.KNOT_B, v)
            dl = dl + pick(kind == tk.KNOT_B, v)
            carry = Fd
            own0["a"] = own0["a"] - pick(p["seg_a"], PAd)
            own0["b"] = own0["b"] + pick(p["seg_b"], PBd)
            dl = dl + PBd
        bar_b = bar_b + carry
        end_a, end_b = walk["cls_b"] == tk.B_END_A, walk["cls_b"] == tk.B_END_B
        for side, own_end in (("a", end_a), ("b", end_b)):
            new = list(sums[side])
            new[12] = (new[12] + own0[side]) + pick(own_end, bar_b)
            new[13] = new[13] + pick(own_end, bar_b)
            sums[side] = new
        lo_bar_dot = pick(walk["cls_a"] == tk.A_LO, bar_a)
        hi_bar_dot = pick(walk["cls_b"] == tk.B_HI, bar_b)
        dl_bar_dot = (dl + pick(walk["cls_a"] == tk.A_START, bar_a)) + pick(end_b, bar_b)
    stack = lambda terms: np.stack([x + zero for x in terms], axis=0)      # noqa: E731
    return stack(sums["a"]), stack(sums["b"]), lo_bar_dot, hi_bar_dot, dl_bar_dot


def _bad(a, b, T):
    return np.isnan(tr._columns(a, T)[6][:, 0]) | np.isnan(tr._columns(b, T)[6][:, 0])


def _finish(a, b, a_dot, b_dot, Sa, Sb, T):
    bad = _bad(a, b, T)
    out = []
    for spline, dot, S in ((a, a_dot, Sa), (b, b_dot, Sb)):
        out.append([np.where(bad, T(np.nan), x) for x in ih._finish(spline, dot, S, T)])
    return out


def hvp_ld(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, delay_dot):
    """(A's eight results, B's eight, lo_bar_dot, hi_bar_dot, delay_bar_dot (n, k) each) in longdouble; g three (n, k) arrays, a_dot and
    b_dot eight arrays of n, lo_dot, hi_dot and delay_dot (n, k) -- None anywhere: zeros."""
    ta, tb, lb, hb, db = _terms(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, delay_dot, LD)
    with np.errstate(all="ignore"):
        bars = _finish(a, b, a_dot, b_dot, ta.sum(axis=2), tb.sum(axis=2), LD)
    return bars[0], bars[1], lb, hb, db


def _lane_sums(terms):
    """(14, n, k) -> (14, n) in reduce_rows' order of additions."""
    _, n, k = terms.shape
    G, vec = tr.group_lanes(k)
    per = 2 if vec else 1
    units = k // per
    S = np.zeros((terms.shape[0], n, G))
    for first in range(0, units, G):
        lanes = np.arange(min(G, units - first))
        for e in range(per):
            S[:, :, lanes] = S[:, :, lanes] + terms[:, :, (first + lanes) * per + e]
    m = 1
    while m < G:
        S = S + S[:, :, np.arange(G) ^ m]
        m *= 2
    return S[:, :, 0]


def hvp_f64(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, delay_dot):
    """The same as k_pair_hvp forms it: float64, a problem's queries added in k_trajectory_vjp's order."""
    ta, tb, lb, hb, db = _terms(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, delay_dot, np.float64)
    with np.errstate(all="ignore"):
        bars = _finish(a, b, a_dot, b_dot, _lane_sums(ta), _lane_sums(tb), np.float64)
    return bars[0], bars[1], lb, hb, db


# ---------------------------------------------------------------- inputs and measures
def _size(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(np.abs(np.where(np.isfinite(x), x, 0.0)), 1.0)


def directions(a, b, lo, hi, delay, seed, scaled=False):
    """A random direction in all nineteen inputs: (a_dot, b_dot eight arrays of n each, lo_dot, hi_dot, delay_dot (n, k)).  With `scaled`
    every component is multiplied by max(|x|, 1) of its input."""
    rng = np.random.default_rng(seed)
    n, shape = len(a[0]), np.shape(delay)
    a_dot, b_dot = [rng.standard_normal(n) for _ in range(8)], [rng.standard_normal(n) for _ in range(8)]
    q = [rng.standard_normal(shape) for _ in range(3)]
    if scaled:
        a_dot = [d * _size(x) for d, x in zip(a_dot, a)]
        b_dot = [d * _size(x) for d, x in zip(b_dot, b)]
        q = [d * _size(x) for d, x in zip(q, (lo, hi, delay))]
    return a_dot, b_dot, q[0], q[1], q[2]


def gradients(shape, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(shape) for _ in range(3)]


def translation(n):
    """pos0_dot = pos1_dot = pos2_dot = 1, everything else 0: the spline moves as a whole."""
    one, zero = np.ones(n), np.zeros(n)
    return [one, one, one, zero, zero, zero, zero, zero]


def flat(result):
    """(A's bars, B's bars, lo_bar_dot, hi_bar_dot, delay_bar_dot) as one list of nineteen arrays, for trajectory_ref.normwise."""
    return list(result[0]) + list(result[1]) + [result[2], result[3], result[4]]


def bilinear(result, direction):
    """u^T (H v) for H v = result and u = direction (both in flat()'s layout before flattening), per problem in longdouble: (the value, the
    sum of |terms|)."""
    value, size = LD(0), LD(0)
    for x, y in zip(flat(result), flat(direction)):
        t = np.asarray(x, dtype=LD) * np.asarray(y, dtype=LD)
        if t.ndim == 2:
            value, size = value + t.sum(axis=1), size + np.abs(t).sum(axis=1)
        else:
            value, size = value + t, size + np.abs(t)
    return value, size
