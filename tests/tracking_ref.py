"""Test-side restatements of the tracking integrals between two splines (rp_trajectory_tracking / _vjp / _jvp, csrc/trajectory.hip;
DESIGN.md section 20), on top of tests/trajectory_ref.py and tests/gap_ref.py, whose domain, window, knots and input families these are: a
spline is its list of eight arrays, a query a window lo, hi and a delay, three (n, k) arrays (None: -inf / +inf / 0).
D(t) = pos_A(t) - pos_B(t - delay); the three outputs are NAMES = (gap_int, gap_sq, relvel_sq), the integrals of D, D^2 and D'^2.

    tracking_ld      the definition in longdouble with true divisions: three (n, k) arrays, NaN where the query has no answer
    tracking_f64     the kernel's rule in float64, operation for operation (1 / h is numpy's division where the kernel has its refined
                     reciprocal, so it restates the rule, not the bits)
    vjp_ld / jvp_ld  the derivative rule -- per piece dI = S mA_i dC_A,i - S mB_i dC_B,i + P_A ds_A - P_B ds_B + f(w) dw, the piece ends'
                     tangents by where each end came from -- in longdouble, plain sums; vjp_f64 / jvp_f64 the same rule in float64
    gauss_ld         the same integrals by 8-point Gauss-Legendre per piece through trajectory_ref.forward_ld: exact for degree 6 and
                     sharing no formula with the closed forms
    identity_defect  per piece and output, (P_A - P_B) - (f(w) - f(0)) over the size of its terms
    value_scales     the three outputs' scales: scale T, scale^2 T, (scale / T)^2 T
    kept_for_differences
                     the queries far enough from every kink for a difference quotient

One code path serves both types: T is np.longdouble or np.float64.
"""
import numpy as np

import gap_ref as gr
import trajectory_ref as tr

LD = np.longdouble
NAMES = ("gap_int", "gap_sq", "relvel_sq")
A_LO, A_START, A_NONE = range(3)            # where the window's a came from
B_HI, B_END_A, B_END_B = range(3)           # ... and its b
END_A, END_B, KNOT_A, KNOT_B = range(4)     # what a piece end is
# The forward bounds, of each output's scale (value_scales): ten times the worst error of tracking_f64 against tracking_ld over the four
# families at n = 512, k = 8 (8.0e-17, 7.3e-17, 2.3e-15; DESIGN.md section 20's table) -- tests/test_tracking_cpu.py measures them again.
FORWARD_BOUNDS = (8.1e-16, 7.4e-16, 2.4e-14)


def value_scales(a, b):
    """(n, 1) each: scale T, scale^2 T, (scale / T)^2 T with scale the larger position scale of the two splines and T = max(T_A, T_B)."""
    sc = gr.scale(a, b)
    T = np.maximum(np.asarray(a[6]) + np.asarray(a[7]), np.asarray(b[6]) + np.asarray(b[7]))[:, None]
    return [sc * T, sc * sc * T, (sc / T) ** 2 * T]


def _constants(spline, T):
    """Per segment a dict of (n, 1) columns of type T: x0, x1, va, vb, h, ih, acc0, jrk0 -- the definition's true divisions in longdouble,
    the kernel's staged constants in float64."""
    p0, p1, p2, v0, v2, v1, d0, d1 = tr._columns(spline, T)
    out = []
    with np.errstate(all="ignore"):
        for x0, x1, va, vb, h in ((p0, p1, v0, v1, d0), (p1, p2, v1, v2, d1)):
            ih = T(1) / h
            if T is LD:
                acc0 = 6 * (x1 - x0) / h**2 - (4 * va + 2 * vb) / h
                jrk0 = 2 * (vb - va) / h**2 - 2 * acc0 / h
            else:
                acc0, jrk0 = tr._constants_f64(x0, x1, va, vb, ih)
            out.append({"x0": x0, "x1": x1, "va": va, "vb": vb, "h": h, "ih": ih, "acc0": acc0, "jrk0": jrk0})
    return out


def _pick(segs, seg, name):
    return np.where(seg, segs[1][name], segs[0][name])


def _local(segs, seg, s, T):
    """(pos, vel, acc, jrk0) of the selected segment at local time s, in the evaluator's expressions."""
    x0, va, acc0, jrk0 = (_pick(segs, seg, f) for f in ("x0", "va", "acc0", "jrk0"))
    third, half = T(1) / T(3), T(0.5)
    return (x0 + (va + (acc0 + jrk0 * (s * third)) * (s * half)) * s, va + (acc0 + jrk0 * (s * half)) * s, acc0 + jrk0 * s, jrk0 + 0 * s)


def _walk(a, b, lo, hi, delay, T):
    """The domain, the clamped window and the three pieces, by gap_query's float64 expressions (the times are float64 values; only the
    arithmetic on them is of type T)."""
    lo, hi, delay = gr._queries(a, lo, hi, delay)
    S, E, kA, kB, TA, EB = gr._domain(a, b, delay)
    with np.errstate(all="ignore"):
        wide = lambda t: np.broadcast_to(t, lo.shape)      # noqa: E731
        S, E, kA, kB, TA, EB = (wide(x) for x in (S, E, kA, kB, TA, EB))
        wa = np.where(lo > S, lo, np.where(np.isnan(lo), lo, S))
        wb = np.where(hi < E, hi, np.where(np.isnan(hi), hi, E))
        ok = (wa <= wb) & np.isfinite(delay) & ~np.isnan(EB)
        cls_a = np.where(lo > S, A_LO, np.where(delay > 0, A_START, A_NONE))
        cls_b = np.where(hi < E, B_HI, np.where(EB < TA, B_END_B, B_END_A))
        b_first = kB < kA
        pieces, c, kind_c = [], wa, np.full(lo.shape, END_A)
        for piece in range(3):
            kb = b_first if piece == 0 else ~b_first
            knot = np.where(kb, kB, kA)
            before, after = knot < wa, knot > wb
            if piece == 2:
                e, kind_e = wb, np.full(lo.shape, END_B)
            else:
                e = np.where(before, wa, np.where(after, wb, knot))
                kind_e = np.where(before, END_A, np.where(after, END_B, np.where(kb, KNOT_B, KNOT_A)))
            seg_a, seg_b = kA <= c, kB <= c
            cT, eT = c.astype(T), e.astype(T)
            pieces.append({"c": c, "e": e, "seg_a": seg_a, "seg_b": seg_b, "kind_c": kind_c, "kind_e": kind_e, "w": eT - cT,
                           "sA": np.where(seg_a, cT - kA.astype(T), cT), "sB": np.where(seg_b, cT - kB.astype(T), cT - delay.astype(T))})
            c, kind_c = e, kind_e
    return {"ok": ok, "empty": ok & (wa == wb), "a": wa, "b": wb, "cls_a": cls_a, "cls_b": cls_b, "pieces": pieces, "delay": delay,
            "S": S, "E": E, "kA": kA, "kB": kB, "lo": lo, "hi": hi}


def _state(ca, cb, p, T):
    XA, VA, AA, JA = _local(ca, p["seg_a"], p["sA"], T)
    XB, VB, AB, JB = _local(cb, p["seg_b"], p["sB"], T)
    return {"X": XA - XB, "V": VA - VB, "A": AA - AB, "J": JA - JB, "VA": VA, "AA": AA, "JA": JA, "VB": VB, "AB": AB, "JB": JB}


def _values(t, w, T):
    """One piece's three contributions, in k_tracking's nesting."""
    X, V, A, J = t["X"], t["V"], t["A"], t["J"]
    third, half = T(1) / T(3), T(0.5)
    v0 = w * (X + (w * half) * (V + (w * third) * (A + (w * T(0.25)) * J)))
    t6 = (A * J) * (T(1) / T(36)) + w * ((J * J) * (T(1) / T(252)))
    t5 = ((A * A) * T(0.25) + (V * J) * third) * (T(1) / T(5)) + w * t6
    t4 = (V * A + (X * J) * third) * T(0.25) + w * t5
    t3 = (V * V + X * A) * third + w * t4
    v1 = w * (X * X + w * (X * V + w * t3))
    v2 = w * (V * V + w * (V * A + (w * third) * ((A * A + V * J) + w * (T(0.75) * (A * J) + ((T(3) / T(20)) * w) * (J * J)))))
    return [v0, v1, v2]


def _tracking(a, b, lo, hi, delay, T):
    walk = _walk(a, b, lo, hi, delay, T)
    ca, cb = _constants(a, T), _constants(b, T)
    with np.errstate(all="ignore"):
        total = [T(0), T(0), T(0)]
        for p in walk["pieces"]:
            v = _values(_state(ca, cb, p, T), p["w"], T)
            total = [total[i] + v[i] for i in range(3)]
        return [np.where(walk["ok"], np.where(walk["empty"], T(0), total[i]), T(np.nan)) for i in range(3)]


def tracking_ld(a, b, lo=None, hi=None, delay=None):
    """Three (n, k) longdouble arrays, NAMES' order: NaN where the query has no answer, +0.0 where a == b."""
    return _tracking(a, b, lo, hi, delay, LD)


def tracking_f64(a, b, lo=None, hi=None, delay=None):
    """The same by the kernel's rule in float64."""
    return _tracking(a, b, lo, hi, delay, np.float64)


_GL = np.polynomial.legendre.leggauss(8)


def gauss_ld(a, b, lo=None, hi=None, delay=None):
    """The three integrals by 8-point Gauss-Legendre on each piece, the integrand through trajectory_ref.forward_ld of each spline."""
    walk = _walk(a, b, lo, hi, delay, LD)
    nodes, weights = (np.asarray(x, dtype=LD) for x in _GL)
    dl = walk["delay"].astype(LD)
    with np.errstate(all="ignore"):
        total = [LD(0) * dl for _ in range(3)]
        for p in walk["pieces"]:
            c, w = p["c"].astype(LD), p["w"]
            for x, wt in zip(nodes, weights):
                t = c + w * (x + 1) / 2
                t = np.where(walk["ok"], t, LD(0))
                pa, va, _ = tr.forward_ld(a, t)
                pb, vb, _ = tr.forward_ld(b, np.where(walk["ok"], t - dl, LD(0)))
                D, Dp = pa - pb, va - vb
                for i, f in enumerate((D, D * D, Dp * Dp)):
                    total[i] = total[i] + f * (wt * w / 2)
        return [np.where(walk["ok"], np.where(walk["empty"], LD(0), total[i]), LD(np.nan)) for i in range(3)]


# ---------------------------------------------------------------- the derivative rule
def _partials(t, p, T):
    """Per output: (mA[4], mB[4], P_A, P_B, f(w), f(0)) of one piece, polynomials in w from the local states at the piece's start."""
    w, X, V, A, J = p["w"], t["X"], t["V"], t["A"], t["J"]
    third, half = T(1) / T(3), T(0.5)
    Dw = X + w * (V + (w * half) * (A + (w * third) * J))
    Vw = V + w * (A + (w * half) * J)
    E = [X * w ** (m + 1) / (m + 1) + V * w ** (m + 2) / (m + 2) + A * w ** (m + 3) / (2 * (m + 3)) + J * w ** (m + 4) / (6 * (m + 4))
         for m in range(4)]
    Q = [V * w ** (m + 1) / (m + 1) + A * w ** (m + 2) / (m + 2) + J * w ** (m + 3) / (2 * (m + 3)) for m in range(3)]
    out = []
    for o in range(3):
        sides = []
        for s, Vs, As, Js in ((p["sA"], t["VA"], t["AA"], t["JA"]), (p["sB"], t["VB"], t["AB"], t["JB"])):
            if o == 0:
                # the integral of (s + u)^m over [0, w], expanded in w so that nothing is differenced
                M = [w, w * (s + w * half), w * (s * s + w * (s + w * third)), w * (s ** 3 + w * (T(1.5) * (s * s) + w * (s + w * T(0.25))))]
                m4 = [M[0], M[1], M[2] * half, M[3] / 6]
                P = w * (Vs + (w * half) * (As + (w * third) * Js))
            elif o == 1:
                m4 = [2 * E[0], 2 * (s * E[0] + E[1]), s * s * E[0] + 2 * s * E[1] + E[2], (s ** 3 * E[0] + E[3]) / 3 + s * s * E[1] + s * E[2]]
                P = 2 * (Vs * E[0] + As * E[1] + Js * E[2] / 2)
            else:
                m4 = [0 * w, 2 * Q[0], 2 * (s * Q[0] + Q[1]), s * s * Q[0] + 2 * s * Q[1] + Q[2]]
                P = 2 * (As * Q[0] + Js * Q[1])
            sides.append((m4, P))
        fw, f0 = ((Dw, X), (Dw * Dw, X * X), (Vw * Vw, V * V))[o]
        out.append((sides[0][0], sides[1][0], sides[0][1], sides[1][1], fw, f0))
    return out


def identity_defect(a, b, lo=None, hi=None, delay=None):
    """(n, k, 3 pieces, 3 outputs) float64: |(P_A - P_B) - (f(w) - f(0))| over |P_A| + |P_B| + |f(w)| + |f(0)|, in longdouble; 0 where the
    query has no answer or every term is 0."""
    walk = _walk(a, b, lo, hi, delay, LD)
    ca, cb = _constants(a, LD), _constants(b, LD)
    out = np.zeros(walk["ok"].shape + (3, 3))
    with np.errstate(all="ignore"):
        for j, p in enumerate(walk["pieces"]):
            for o, (_, _, PA, PB, fw, f0) in enumerate(_partials(_state(ca, cb, p, LD), p, LD)):
                size = np.abs(PA) + np.abs(PB) + np.abs(fw) + np.abs(f0)
                d = np.where(walk["ok"] & (size > 0), np.abs((PA - PB) - (fw - f0)) / np.where(size > 0, size, LD(1)), LD(0))
                out[..., j, o] = np.asarray(d, dtype=np.float64)
    return out


def _chain(seg, Sx, Sv, Sa, Sj):
    """segment_chain: the gradients on (x0, va, acc0, jrk0) of one segment to (x0, x1, va, vb, h), arrays of n."""
    x0, x1, va, vb, ih, acc0 = (seg[f][:, 0] for f in ("x0", "x1", "va", "vb", "ih", "acc0"))
    ih2 = ih * ih
    ih3 = ih2 * ih
    A = Sa - (2 * ih) * Sj
    x1b = (6 * ih2) * A
    return (Sx - x1b, x1b, Sv - (4 * ih) * A - (2 * ih2) * Sj, (2 * ih2) * Sj - (2 * ih) * A,
            A * ((va * 4 + vb * 2) * ih2 - (x1 - x0) * (12 * ih3)) + Sj * (acc0 * (2 * ih2) - (vb - va) * (4 * ih3)))


def _vjp(a, b, lo, hi, delay, g, T):
    walk = _walk(a, b, lo, hi, delay, T)
    ca, cb = _constants(a, T), _constants(b, T)
    ok = walk["ok"]
    zero = np.zeros(ok.shape, dtype=T)
    g = [zero if x is None else np.where(ok, np.asarray(x, dtype=T), T(0)) for x in g]
    live = lambda x: np.where(ok, x, T(0))      # noqa: E731
    sums = {side: [[zero, zero, zero, zero], [zero, zero, zero, zero]] for side in "ab"}
    dur = {"a0": zero, "a1": zero, "b0": zero, "b1": zero}
    lo_bar, hi_bar, dl_bar = zero, zero, zero

    def route(kind, v):
        nonlocal lo_bar, hi_bar, dl_bar
        at_a, at_b = kind == END_A, kind == END_B
        end_a, end_b = at_b & (walk["cls_b"] == B_END_A), at_b & (walk["cls_b"] == B_END_B)
        lo_bar = lo_bar + np.where(at_a & (walk["cls_a"] == A_LO), v, T(0))
        hi_bar = hi_bar + np.where(at_b & (walk["cls_b"] == B_HI), v, T(0))
        dl_bar = dl_bar + np.where((at_a & (walk["cls_a"] == A_START)) | end_b | (kind == KNOT_B), v, T(0))
        dur["a0"] = dur["a0"] + np.where(end_a | (kind == KNOT_A), v, T(0))
        dur["a1"] = dur["a1"] + np.where(end_a, v, T(0))
        dur["b0"] = dur["b0"] + np.where(end_b | (kind == KNOT_B), v, T(0))
        dur["b1"] = dur["b1"] + np.where(end_b, v, T(0))

    with np.errstate(all="ignore"):
        for p in walk["pieces"]:
            parts = _partials(_state(ca, cb, p, T), p, T)
            WA = [live(sum(g[o] * parts[o][0][i] for o in range(3))) for i in range(4)]
            WB = [live(-sum(g[o] * parts[o][1][i] for o in range(3))) for i in range(4)]
            PA, PB, F = (live(sum(g[o] * parts[o][j] for o in range(3))) for j in (2, 3, 4))
            for side, W, seg in (("a", WA, p["seg_a"]), ("b", WB, p["seg_b"])):
                for i in range(4):
                    sums[side][0][i] = sums[side][0][i] + np.where(seg, T(0), W[i])
                    sums[side][1][i] = sums[side][1][i] + np.where(seg, W[i], T(0))
            route(p["kind_c"], (PA - PB) - F)      # ds_A = dc - doff_A, ds_B = dc - doff_B, dw = de - dc
            route(p["kind_e"], F)
            dur["a0"] = dur["a0"] - np.where(p["seg_a"], PA, T(0))
            dur["b0"] = dur["b0"] + np.where(p["seg_b"], PB, T(0))
            dl_bar = dl_bar + PB
        bars = []
        for side, consts in (("a", ca), ("b", cb)):
            s0 = _chain(consts[0], *[x.sum(axis=1) for x in sums[side][0]])
            s1 = _chain(consts[1], *[x.sum(axis=1) for x in sums[side][1]])
            bars.append([s0[0], s0[1] + s1[0], s1[1], s0[2], s1[3], s0[3] + s1[2], s0[4] + dur[side + "0"].sum(axis=1),
                         s1[4] + dur[side + "1"].sum(axis=1)])
    return bars[0], bars[1], lo_bar, hi_bar, dl_bar


def vjp_ld(a, b, lo, hi, delay, g):
    """Reverse mode in longdouble: (A's eight gradients, B's eight, lo_bar, hi_bar, delay_bar (n, k) each) for the upstream gradients g
    (three (n, k) arrays or None); a query without an answer counts with gradients of zero."""
    return _vjp(a, b, lo, hi, delay, g, LD)


def vjp_f64(a, b, lo, hi, delay, g):
    """The same rule in float64."""
    return _vjp(a, b, lo, hi, delay, g, np.float64)


def _tangents(seg, dxd, x0d, vad, vbd, hd):
    """segment_tangents: the tangents of (x0, va, acc0, jrk0)."""
    ih, acc0 = seg["ih"], seg["acc0"]
    ih2 = ih * ih
    ih3 = ih2 * ih
    acc0d = dxd * (6 * ih2) - (seg["x1"] - seg["x0"]) * (12 * ih3) * hd - (vad * 4 + vbd * 2) * ih + (seg["va"] * 4 + seg["vb"] * 2) * ih2 * hd
    jrk0d = (vbd - vad) * (2 * ih2) - (seg["vb"] - seg["va"]) * (4 * ih3) * hd - acc0d * (2 * ih) + acc0 * (2 * ih2) * hd
    return [x0d, vad, acc0d, jrk0d]


def _jvp(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot, T):
    walk = _walk(a, b, lo, hi, delay, T)
    ca, cb = _constants(a, T), _constants(b, T)
    shape = walk["ok"].shape
    col = lambda x: np.zeros((shape[0], 1), dtype=T) if x is None else np.asarray(x, dtype=T)[:, None]      # noqa: E731
    full = lambda x: np.zeros(shape, dtype=T) if x is None else np.asarray(x, dtype=T)      # noqa: E731
    da, db = [col(x) for x in (a_dot or [None] * 8)], [col(x) for x in (b_dot or [None] * 8)]
    lod, hid, dld = full(lo_dot), full(hi_dot), full(delay_dot)
    with np.errstate(all="ignore"):
        tan = {}
        for side, c, d in (("a", ca, da), ("b", cb, db)):
            tan[side] = [_tangents(c[0], d[1] - d[0], d[0], d[3], d[5], d[6]), _tangents(c[1], d[2] - d[1], d[1], d[5], d[4], d[7])]
        ad = np.where(walk["cls_a"] == A_LO, lod, np.where(walk["cls_a"] == A_START, dld, T(0)))
        bd = np.where(walk["cls_b"] == B_HI, hid, np.where(walk["cls_b"] == B_END_A, da[6] + da[7], dld + (db[6] + db[7])))
        kAd, kBd = da[6] + 0 * dld, dld + db[6]
        tangent = lambda kind: np.where(kind == END_A, ad, np.where(kind == END_B, bd, np.where(kind == KNOT_A, kAd, kBd)))      # noqa: E731
        total = [np.zeros(shape, dtype=T) for _ in range(3)]
        for p in walk["pieces"]:
            cd, ed = tangent(p["kind_c"]), tangent(p["kind_e"])
            dsA = cd - np.where(p["seg_a"], kAd, T(0))
            dsB = cd - np.where(p["seg_b"], kBd, dld)
            dw = ed - cd
            dCA = [np.where(p["seg_a"], tan["a"][1][i], tan["a"][0][i]) for i in range(4)]
            dCB = [np.where(p["seg_b"], tan["b"][1][i], tan["b"][0][i]) for i in range(4)]
            for o, (mA, mB, PA, PB, fw, _) in enumerate(_partials(_state(ca, cb, p, T), p, T)):
                first = 1 if o == 2 else 0      # a partial that is 0 by structure is not a term
                lead = sum(mA[i] * dCA[i] for i in range(first, 4)) - sum(mB[i] * dCB[i] for i in range(first, 4))
                total[o] = total[o] + (lead + (PA * dsA - PB * dsB) + fw * dw)
        return [np.where(walk["ok"], x, T(np.nan)) for x in total]


def jvp_ld(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot):
    """Forward mode in longdouble: the three outputs' tangents (n, k), NaN where the output is, for tangents on both splines' eight inputs
    (lists of arrays of n, None entries or None: zeros) and on lo, hi, delay ((n, k) or None)."""
    return _jvp(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot, LD)


def jvp_f64(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot):
    """The same rule in float64."""
    return _jvp(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot, np.float64)


def kept_for_differences(a, b, lo, hi, delay, margin=1e-3):
    """(n, k) bool: the queries with an answer whose finite lo, hi lie at least margin T from S, E, both knots and each other, whose knots lie
    that far from each other, and whose delay is not exactly 0 -- T = max(T_A, T_B)."""
    walk = _walk(a, b, lo, hi, delay, np.float64)
    T = np.maximum(np.asarray(a[6]) + np.asarray(a[7]), np.asarray(b[6]) + np.asarray(b[7]))[:, None]
    tol = margin * T
    keep = walk["ok"] & ~walk["empty"] & (walk["delay"] != 0)
    with np.errstate(all="ignore"):
        keep &= np.abs(walk["kA"] - walk["kB"]) >= tol
        for end in (walk["lo"], walk["hi"]):
            fin = np.isfinite(end)
            for ref in (walk["S"], walk["E"], walk["kA"], walk["kB"]):
                keep &= ~fin | (np.abs(end - ref) >= tol)
        both = np.isfinite(walk["lo"]) & np.isfinite(walk["hi"])
        keep &= ~both | (np.abs(walk["hi"] - walk["lo"]) >= tol)
    return keep


# ---------------------------------------------------------------- inputs
def family(name, n=512, k=8):
    """(A, B, lo, hi, delay) of one of section 18's families: random, solved, follower (delayed), follower0 (the solved A against itself
    lowered by 25 at a delay of exactly 0)."""
    if name == "random":
        a, b = gr.random_pair(n)
        delay = gr.delays(a, b, k, 11)
    elif name == "solved":
        a, b = gr.solved_pair(n)
        delay = gr.delays(a, b, k, 12)
    elif name == "follower":
        a = gr.solved_pair(n)[0]
        b = gr.follower(a)
        delay = gr.delays(a, b, k, 13, follow=True)
    elif name == "follower0":
        a = gr.solved_pair(n)[0]
        b = gr.follower(a)
        delay = np.zeros((n, k))
    else:
        raise ValueError(name)
    lo, hi = gr.windows(a, b, delay, 21)
    return a, b, lo, hi, delay


FAMILIES = ("random", "solved", "follower", "follower0")


def dyadic_cases():
    """(A, B, lo, hi, delay, expected (4, 3)): gap_ref.knot_cases' four dyadic pairs with a window end exactly on k_A (case 0: [0.5, 1]), on
    k_B = delay + duration0_B with delay = 0.25 (case 1: [1.25, +inf)), on the START (case 2: (-inf, 1], a = delay = 0.5) and on END_B (case 3:
    [1, +inf), b = delay + T_B = 2.5).  Every time, constant and local state is a dyadic rational that float64 holds exactly, so the two
    restatements differ only by the rounding of the polynomials' own constants (1 / 3, 1 / 36, 1 / 252, ...)."""
    a, b, _, _, delay, _ = gr.knot_cases()
    lo = np.array([[0.5], [1.25], [-np.inf], [1.0]])
    hi = np.array([[1.0], [np.inf], [1.0], [np.inf]])
    return a, b, lo, hi, delay
