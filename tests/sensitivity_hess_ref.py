"""Test-side restatements of the second derivative of an F3 solution with respect to the positions (rp_batch_solution_hessian;
DESIGN.md section 12).

For an F3 state z = (x, lam), x = (vel1, duration0, duration1), positions theta = (pos0, pos1, pos2) and tangents u, w:
    M z_u = -(dr/dtheta) u,    M z_uw = -R_uw
with R_uw the second total derivative of r along (z_u, u), (z_w, w), every z_uw term left out.  r depends on theta only through
dX0 = pos1 - pos0 and dX1 = pos2 - pos1, so the three (dX, dX) pairs give every x_uw, and H[a][b][c] = d^2 x_a / dpos_b dpos_c
follows through P = d dX / d pos = [[-1, 1, 0], [0, -1, 1]].

full_hessian solves both systems on the full 11 x 11 matrix in np.longdouble, with R_uw written from the residual's definition
(every multiplier's own first-order step, no condensation) and the accelerations' derivative tables below.  condensed_hessian
restates the kernel's arithmetic in float64: the first-order steps from the 7 x 7 active-set-aware system (each pair's dual step
an unknown of the row h_j . x - mu_j / D_j = -alpha_j), the three second-order right-hand sides on the VJP's condensed 3 x 3 K in
double-double, both eliminations with the kernel's pivot order.  naive_hessian is the rejected form: the first-order steps from K, and
mu_j,u = D_j A_j,u formed from them.
"""
import numpy as np

import sensitivity_jvp_ref as jr
import sensitivity_ref as sr

LD = np.longdouble
L_DEFAULT = 100.0
SIGMA = (1, -1, 1, -1)      # sign of the dX term of a_j: a_j = 6 sigma_j dX / t^2 + w_j / t
CV = (-2, 4, -4, 2)         # d w_j / d vel1 of the velocity combinations w_j = m0, n0, m1, n1
P = np.array([[-1, 1, 0], [0, -1, 1]])      # d (dX0, dX1) / d (pos0, pos1, pos2)


def accel_tables(states, dtype=LD):
    """a_j and every non-zero derivative of a_j in (v, t, dX) of its segment, (n, 4) each, in `dtype`.  The third derivatives
    needed are a_ttt, a_vtt, a_Xtt; a_vv, a_XX, a_vX and everything built on them vanish."""
    s = np.asarray(states, dtype=dtype)
    v, t0, t1 = s[:, 0], s[:, 1], s[:, 2]
    v0, v2 = s[:, 12], s[:, 15]
    dx0, dx1 = s[:, 13] - s[:, 11], s[:, 14] - s[:, 13]
    w = np.stack([-4 * v0 - 2 * v, 2 * v0 + 4 * v, -4 * v - 2 * v2, 2 * v + 4 * v2], axis=1)
    r = np.stack([1 / t0, 1 / t0, 1 / t1, 1 / t1], axis=1)
    X = np.stack([dx0, dx0, dx1, dx1], axis=1)
    sg = np.asarray(SIGMA, dtype=dtype)
    cv = np.asarray(CV, dtype=dtype)
    return dict(
        a=6 * sg * X * r**2 + w * r,
        v=cv * r, t=-12 * sg * X * r**3 - w * r**2, X=6 * sg * r**2,
        tt=36 * sg * X * r**4 + 2 * w * r**3, vt=-cv * r**2, Xt=-12 * sg * r**3,
        ttt=-144 * sg * X * r**5 - 6 * w * r**4, vtt=2 * cv * r**3, Xtt=36 * sg * r**4)


def kkt_ld(states, limit=L_DEFAULT):
    """M = dr/dz (n, 11, 11) in longdouble from the derivative tables: r_x = grad f + S_i lam_i grad c_i, r_i = lam_i c_i + p with
    c_2j = -a_j - L, c_2j+1 = a_j - L (the oracle's kkt() in float64 is the same matrix)."""
    s = np.asarray(states, dtype=LD)
    n = len(s)
    T = accel_tables(s)
    lam = s[:, 3:11]
    mu = lam[:, 1::2] - lam[:, 0::2]
    M = np.zeros((n, 11, 11), dtype=LD)
    for j in range(4):
        seg = 1 + (j >> 1)
        M[:, 0, seg] += mu[:, j] * T["vt"][:, j]
        M[:, seg, 0] += mu[:, j] * T["vt"][:, j]
        M[:, seg, seg] += mu[:, j] * T["tt"][:, j]
    for i in range(8):
        j, sgn = i >> 1, (1 if i & 1 else -1)
        seg = 1 + (j >> 1)
        c = sgn * T["a"][:, j] - limit
        M[:, 0, 3 + i] = sgn * T["v"][:, j]
        M[:, seg, 3 + i] = sgn * T["t"][:, j]
        M[:, 3 + i, 0] = lam[:, i] * sgn * T["v"][:, j]
        M[:, 3 + i, seg] = lam[:, i] * sgn * T["t"][:, j]
        M[:, 3 + i, 3 + i] = c
    return M


def residual_ld(states, p, limit=L_DEFAULT):
    """r(z; theta, p) (n, 11) in longdouble: the residual whose M kkt_ld is; p (n,) held fixed."""
    s = np.asarray(states, dtype=LD)
    T = accel_tables(s)
    lam = s[:, 3:11]
    mu = lam[:, 1::2] - lam[:, 0::2]
    r = np.zeros((len(s), 11), dtype=LD)
    r[:, 0] = np.sum(mu * T["v"], axis=1)
    r[:, 1] = 1 + mu[:, 0] * T["t"][:, 0] + mu[:, 1] * T["t"][:, 1]
    r[:, 2] = 1 + mu[:, 2] * T["t"][:, 2] + mu[:, 3] * T["t"][:, 3]
    for i in range(8):
        sgn = 1 if i & 1 else -1
        r[:, 3 + i] = lam[:, i] * (sgn * T["a"][:, i >> 1] - limit) + np.asarray(p, dtype=LD)
    return r


def first_order(M, states):
    """z_u (n, 2, 11) longdouble for u = the unit dX0 and dX1 tangents: M z_u = -(dr/d dX) u."""
    D = sr.drdtheta(states)      # columns pos0, pos1, pos2; the dX columns are -col(pos0) and col(pos2)
    ddx = np.stack([-D[:, :, 0], D[:, :, 2]], axis=2)
    M = np.asarray(M, dtype=LD)
    return np.stack([sr.solve_batched(M, -ddx[:, :, u]) for u in range(2)], axis=1)


def second_rhs(states, zu, limit=L_DEFAULT):
    """R_uw (n, 3, 11) longdouble for (u, w) = (0, 0), (0, 1), (1, 1), from the definition: every multiplier's own first-order
    step lam_i,u, the constraint values' total derivatives c_i,u and c_i,uw (without x_uw), the x rows' S_i lam_i grad c_i
    differentiated twice."""
    s = np.asarray(states, dtype=LD)
    n = len(s)
    T = accel_tables(s)
    lam = s[:, 3:11]
    out = np.zeros((n, 3, 11), dtype=LD)
    for k, (u, w) in enumerate(((0, 0), (0, 1), (1, 1))):
        R = out[:, k]
        for i in range(8):
            j, sgn = i >> 1, (1 if i & 1 else -1)
            seg = j >> 1
            yu = [zu[:, u, 0], zu[:, u, 1 + seg], np.full(n, LD(seg == u))]      # (v, t, dX) tangents of a_j's arguments
            yw = [zu[:, w, 0], zu[:, w, 1 + seg], np.full(n, LD(seg == w))]
            lu, lw = zu[:, u, 3 + i], zu[:, w, 3 + i]
            g = lambda y: T["v"][:, j] * y[0] + T["t"][:, j] * y[1] + T["X"][:, j] * y[2]      # noqa: E731  d a_j along y
            # d (grad_x a_j) along y: (a_vt t, a_tt t + a_vt v + a_Xt X)
            hv = lambda y: T["vt"][:, j] * y[1]      # noqa: E731
            ht = lambda y: T["tt"][:, j] * y[1] + T["vt"][:, j] * y[0] + T["Xt"][:, j] * y[2]      # noqa: E731
            Q = (T["tt"][:, j] * yu[1] * yw[1] + T["vt"][:, j] * (yu[0] * yw[1] + yw[0] * yu[1])
                 + T["Xt"][:, j] * (yu[2] * yw[1] + yw[2] * yu[1]))
            T3v = T["vtt"][:, j] * yu[1] * yw[1]
            T3t = (T["ttt"][:, j] * yu[1] * yw[1] + T["vtt"][:, j] * (yu[0] * yw[1] + yw[0] * yu[1])
                   + T["Xtt"][:, j] * (yu[2] * yw[1] + yw[2] * yu[1]))
            # x rows: (lam_i sgn grad_x a_j)_uw without lam_uw and x_uw
            R[:, 0] += sgn * (lu * hv(yw) + lw * hv(yu) + lam[:, i] * T3v)
            R[:, 1 + seg] += sgn * (lu * ht(yw) + lw * ht(yu) + lam[:, i] * T3t)
            # complementarity: (lam_i c_i)_uw without lam_uw c_i and lam_i grad c_i . x_uw
            R[:, 3 + i] = lu * sgn * g(yw) + lw * sgn * g(yu) + lam[:, i] * sgn * Q
    return out


def _H_from_pairs(xuw):
    """H (n, 3, 3, 3) from x_uw (n, 3, 3) = x for (u, w) = (0, 0), (0, 1), (1, 1): H[a] = P^T [[x00, x01], [x01, x11]] P,
    assembled as the kernel does (each (b, c) entry formed once and written to both places: symmetric exactly)."""
    x00, x01, x11 = xuw[:, 0], xuw[:, 1], xuw[:, 2]
    h01, h12 = x01 - x00, x01 - x11
    H = np.zeros((len(xuw), 3, 3, 3), dtype=xuw.dtype)
    for (b, c), val in (((0, 0), x00), ((0, 1), h01), ((0, 2), -x01), ((1, 1), -h01 - h12), ((1, 2), h12), ((2, 2), x11)):
        H[:, :, b, c] = H[:, :, c, b] = val
    return H


def full_hessian(states, M=None, orc=None, limit=L_DEFAULT):
    """(J (n, 3, 3), H (n, 3, 3, 3)) longdouble from the full 11 x 11 system.  M: the Newton matrix at `states` (default: the
    oracle's kkt() when `orc` is given, else kkt_ld)."""
    if M is None:
        M = sr.kkt_batch(orc, states) if orc is not None else kkt_ld(states, limit)
    M = np.asarray(M, dtype=LD)
    zu = first_order(M, states)
    R = second_rhs(states, zu, limit)
    xuw = np.stack([sr.solve_batched(M, -R[:, k])[:, :3] for k in range(3)], axis=1)
    d0, d1 = zu[:, 0, :3], zu[:, 1, :3]
    J = np.stack([-d0, d0 - d1, d1], axis=2)
    return J, _H_from_pairs(xuw)


def gepp(A, B):
    """X with A X = B, A (n, m, m), B (n, m, r), float64: the kernels' elimination -- for each column k the rows below are
    compared with row k in turn and swapped in when larger (the pivot is the column's largest magnitude), then eliminated."""
    A = np.array(A, dtype=np.float64)
    B = np.array(B, dtype=np.float64)
    m = A.shape[1]
    with np.errstate(all="ignore"):
        for k in range(m - 1):
            for r in range(k + 1, m):
                sw = np.abs(A[:, r, k]) > np.abs(A[:, k, k])
                Ak, Ar = A[:, k].copy(), A[:, r].copy()
                A[:, k] = np.where(sw[:, None], Ar, Ak)
                A[:, r] = np.where(sw[:, None], Ak, Ar)
                Bk, Br = B[:, k].copy(), B[:, r].copy()
                B[:, k] = np.where(sw[:, None], Br, Bk)
                B[:, r] = np.where(sw[:, None], Bk, Br)
            for r in range(k + 1, m):
                f = A[:, r, k] / A[:, k, k]
                A[:, r, k + 1:] -= f[:, None] * A[:, k, k + 1:]
                B[:, r] -= f[:, None] * B[:, k]
        X = np.zeros_like(B)
        for k in range(m - 1, -1, -1):
            acc = B[:, k].copy()
            for c in range(k + 1, m):
                acc -= A[:, k, c][:, None] * X[:, c]
            X[:, k] = acc / A[:, k, k][:, None]
    return X


def _pair_terms(states, limit):
    """The condensed system (sensitivity_jvp_ref.condensed) and float64 derivative tables, E_j / D_j^2 included."""
    c = jr.condensed_dd(states, limit)
    T = accel_tables(states, np.float64)
    s = np.asarray(states, dtype=np.float64)
    lam = s[:, 3:11]
    floor = limit * jr.C_FLOOR
    with np.errstate(all="ignore"):
        cm = np.maximum(-(-T["a"] - limit), floor)      # |c| of each pair's two constraints, floored as D is
        cp = np.maximum(-(T["a"] - limit), floor)
        E = lam[:, 1::2] / (cp * cp) - lam[:, 0::2] / (cm * cm)
        d2 = c["D"] * c["D"]
        # 0 where D_j^2 is 0 or below the normal range (multipliers of 0 or ~1e-160): the term is ~lam there
        c["ED2"] = np.where(d2 >= np.finfo(np.float64).tiny, E / d2, 0.0)
    c["T"] = T
    return c


def aware_first_order(c):
    """(x_u (n, 2, 3), mu_u (n, 2, 4)) float64 from the 7 x 7 active-set-aware system
        [[W, H^T], [H, -diag(1 / D)]] [x_u; mu_u] = [-b_x; -alpha_u]."""
    n = len(c["ok"])
    T, D, mu, gv, gt = c["T"], c["D"], c["mu"], c["gv"], c["gt"]
    A = np.zeros((n, 7, 7))
    A[:, 0, 1] = A[:, 1, 0] = mu[:, 0] * T["vt"][:, 0] + mu[:, 1] * T["vt"][:, 1]
    A[:, 0, 2] = A[:, 2, 0] = mu[:, 2] * T["vt"][:, 2] + mu[:, 3] * T["vt"][:, 3]
    A[:, 1, 1] = mu[:, 0] * T["tt"][:, 0] + mu[:, 1] * T["tt"][:, 1]
    A[:, 2, 2] = mu[:, 2] * T["tt"][:, 2] + mu[:, 3] * T["tt"][:, 3]
    with np.errstate(all="ignore"):
        for j in range(4):
            seg = 1 + (j >> 1)
            A[:, 0, 3 + j] = A[:, 3 + j, 0] = gv[:, j]
            A[:, seg, 3 + j] = A[:, 3 + j, seg] = gt[:, j]
            A[:, 3 + j, 3 + j] = -1 / np.maximum(D[:, j], np.finfo(np.float64).tiny)
        B = np.zeros((n, 7, 2))
        q0, q1 = c["r0"] ** 2, c["r1"] ** 2
        B[:, 1, 0] = -(12 * q0 * c["r0"] * (mu[:, 1] - mu[:, 0]))
        B[:, 2, 1] = -(12 * q1 * c["r1"] * (mu[:, 3] - mu[:, 2]))
        for j in range(4):
            B[:, 3 + j, j >> 1] = -(6 * SIGMA[j] * (q0 if j < 2 else q1))
    X = gepp(A, B)
    return np.transpose(X[:, :3], (0, 2, 1)), np.transpose(X[:, 3:], (0, 2, 1))


def second_order_condensed(c, xu, muu):
    """x_uw (n, 3, 3) float64 for (u, w) = (0, 0), (0, 1), (1, 1): K x_uw = -T_uw - S_j h_j (D_j Q_j + 2 (E_j / D_j^2) mu_u mu_w),
    K and the right-hand sides in double-double (D_j Q_j exactly), as k_solution_hessian forms them."""
    T, D, mu, gv, gt, ED2 = c["T"], c["D"], c["mu"], c["gv"], c["gt"], c["ED2"]
    B = []
    with np.errstate(all="ignore"):
        for k, (u, w) in enumerate(((0, 0), (0, 1), (1, 1))):
            S = [jr.dd(np.zeros(len(D))) for _ in range(3)]
            for j in range(4):
                seg = j >> 1
                vu, tu, Xu = xu[:, u, 0], xu[:, u, 1 + seg], float(seg == u)
                vw, tw, Xw = xu[:, w, 0], xu[:, w, 1 + seg], float(seg == w)
                tt, vt, Xt = tu * tw, vu * tw + vw * tu, Xu * tw + Xw * tu
                Q = T["tt"][:, j] * tt + T["vt"][:, j] * vt + T["Xt"][:, j] * Xt
                Tv = mu[:, j] * (T["vtt"][:, j] * tt)
                Tt = mu[:, j] * (T["ttt"][:, j] * tt + T["vtt"][:, j] * vt + T["Xtt"][:, j] * Xt)
                hv_u, hv_w = T["vt"][:, j] * tu, T["vt"][:, j] * tw
                ht_u = T["tt"][:, j] * tu + T["vt"][:, j] * vu + T["Xt"][:, j] * Xu
                ht_w = T["tt"][:, j] * tw + T["vt"][:, j] * vw + T["Xt"][:, j] * Xw
                s = jr.dd_add(jr.dd_prod(D[:, j], Q), jr.dd(2 * ED2[:, j] * muu[:, u, j] * muu[:, w, j]))
                S[0] = jr.dd_sub(S[0], jr.dd_add(jr.dd(muu[:, u, j] * hv_w + muu[:, w, j] * hv_u + Tv), jr.dd_mul_d(s, gv[:, j])))
                S[1 + seg] = jr.dd_sub(S[1 + seg], jr.dd_add(jr.dd(muu[:, u, j] * ht_w + muu[:, w, j] * ht_u + Tt),
                                                            jr.dd_mul_d(s, gt[:, j])))
            B.append(S)
    return jr._hi(jr.gepp_dd(c["Kdd"], B))


def _assemble(c, xu, xuw):
    d0, d1 = xu[:, 0], xu[:, 1]
    J = np.stack([-d0, d0 - d1, d1], axis=2)
    H = _H_from_pairs(xuw)
    J[~c["ok"]] = np.nan
    H[~c["ok"]] = np.nan
    return J, H


def condensed_hessian(states, limit=L_DEFAULT):
    """(J (n, 3, 3), H (n, 3, 3, 3)) float64 as k_solution_hessian forms them; NaN for non-finite or infeasible states."""
    c = _pair_terms(states, limit)
    xu, muu = aware_first_order(c)
    return _assemble(c, xu, second_order_condensed(c, xu, muu))


def naive_dual_steps(c):
    """(x_u (n, 2, 3), mu_u (n, 2, 4)) of the rejected form: x_u from the condensed K (the Jacobian kernel's solve) and
    mu_j,u = D_j A_j,u formed from it."""
    n = len(c["ok"])
    one, zero = np.ones(n), np.zeros(n)
    with np.errstate(all="ignore"):
        rhs = np.stack([jr.forward_rhs(c, one, zero), jr.forward_rhs(c, zero, one)], axis=2)
        xu = np.transpose(gepp(c["K"], rhs), (0, 2, 1))
        T = c["T"]
        muu = np.zeros((n, 2, 4))
        for u in range(2):
            for j in range(4):
                seg = j >> 1
                A = T["v"][:, j] * xu[:, u, 0] + T["t"][:, j] * xu[:, u, 1 + seg] + T["X"][:, j] * float(seg == u)
                muu[:, u, j] = c["D"][:, j] * A
    return xu, muu


def naive_hessian(states, limit=L_DEFAULT):
    """The Hessian built on naive_dual_steps."""
    c = _pair_terms(states, limit)
    xu, muu = naive_dual_steps(c)
    return _assemble(c, xu, second_order_condensed(c, xu, muu))


def resolve_ld(states, p, pos, limit=L_DEFAULT, iters=8):
    """Newton on r(z; theta, p) = 0 in longdouble from `states` with the positions replaced by pos (n, 3): the central-path point
    at fixed p.  Returns the longdouble states and the final residual's max norm per problem."""
    s = np.array(states, dtype=LD)
    pos = np.asarray(pos, dtype=LD)
    s[:, 11], s[:, 13], s[:, 14] = pos[:, 0], pos[:, 1], pos[:, 2]
    for _ in range(iters):
        r = residual_ld(s, p, limit)
        dz = sr.solve_batched(kkt_ld(s, limit), -r)
        s[:, :11] += dz
    return s, np.max(np.abs(residual_ld(s, p, limit)), axis=1)
