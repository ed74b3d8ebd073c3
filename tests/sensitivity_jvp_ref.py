"""Test-side restatements of the forward-mode derivative of an F3 solution (rp_batch_solution_jvp, rp_batch_solution_jacobian;
DESIGN.md section 12).

For an F3 state z = (x, lam) and position tangents theta_dot = (pos0_dot, pos1_dot, pos2_dot):
    M z_dot = -(dr/dtheta) theta_dot,    x_dot = z_dot[:3]
full_jvp solves this 11 x 11 system in np.longdouble with M from the oracle (Oracle.kkt) and dr/dtheta from
tests/sensitivity_ref.drdtheta.  condensed_vjp / condensed_jvp / condensed_jacobian restate the kernels' condensed 3 x 3 form (the same
D_j, mu_j, NaN rule, double-double K and right-hand side, and elimination order as csrc/sensitivity.hip), so the accuracy of the
condensation can be measured on the CPU.  condensed() is the float64 K of the rejected naive form (tests/sensitivity_hess_ref.py).
"""
import numpy as np

import sensitivity_ref as sr

LD = np.longdouble
L_DEFAULT = 100.0
C_FLOOR = 8.673617379884035e-19      # c_floor / L: eps / 256


def full_jvp(orc, states, tdot):
    """x_dot (n, 3) longdouble for position tangents tdot (n, 3): the full 11 x 11 system."""
    M = sr.kkt_batch(orc, states)
    rhs = -np.einsum("nij,nj->ni", sr.drdtheta(states), np.asarray(tdot, dtype=LD))
    return sr.solve_batched(M, rhs)[:, :3]


def full_jacobian(orc, states):
    """d(vel1, duration0, duration1) / d(pos0, pos1, pos2) (n, 3, 3) longdouble, column b = full_jvp with tdot = e_b."""
    M = sr.kkt_batch(orc, states)
    D = sr.drdtheta(states)
    return np.stack([sr.solve_batched(M, -D[:, :, b])[:, :3] for b in range(3)], axis=2)


def condensed(states, limit=L_DEFAULT):
    """The kernels' condensed system: dict of K (n, 3, 3), D, mu, gv, gt (n, 4), r0, r1 (n,), ok (n,), cmax (n,: the largest
    constraint value) -- float64."""
    s = np.asarray(states, dtype=np.float64)
    v, t0, t1 = s[:, 0], s[:, 1], s[:, 2]
    lam = s[:, 3:11]
    v0, v2 = s[:, 12], s[:, 15]
    dx0, dx1 = s[:, 13] - s[:, 11], s[:, 14] - s[:, 13]
    r0, r1 = 1 / t0, 1 / t1
    q0, q1 = r0 * r0, r1 * r1
    u0, u1 = dx0 * r0, dx1 * r1
    m0, n0 = -4 * v0 - 2 * v, 2 * v0 + 4 * v      # segment 0: (vel0, vel1)
    m1, n1 = -4 * v - 2 * v2, 2 * v + 4 * v2      # segment 1: (vel1, vel2)
    a = np.stack([(6 * u0 + m0) * r0, (-6 * u0 + n0) * r0, (6 * u1 + m1) * r1, (-6 * u1 + n1) * r1], axis=1)
    gt = np.stack([(-12 * u0 - m0) * q0, (12 * u0 - n0) * q0, (-12 * u1 - m1) * q1, (12 * u1 - n1) * q1], axis=1)
    gv = np.stack([-2 * r0, 4 * r0, -4 * r1, 2 * r1], axis=1)
    htt = np.stack([(36 * u0 + 2 * m0) * q0 * r0, (-36 * u0 + 2 * n0) * q0 * r0,
                    (36 * u1 + 2 * m1) * q1 * r1, (-36 * u1 + 2 * n1) * q1 * r1], axis=1)
    htv = np.stack([2 * q0, -4 * q0, 4 * q1, -2 * q1], axis=1)
    cm, cp = -a - limit, a - limit
    lm, lp = lam[:, 0::2], lam[:, 1::2]
    floor = limit * C_FLOOR
    with np.errstate(all="ignore"):
        D = lp / np.maximum(-cp, floor) + lm / np.maximum(-cm, floor)
        ok = np.all(np.isfinite(s), axis=1) & np.all(~(cm > 0) & ~(cp > 0), axis=1)
        mu = lp - lm
        K = np.zeros((len(s), 3, 3))
        K[:, 0, 0] = np.sum(D * gv * gv, axis=1)
        K[:, 0, 1] = K[:, 1, 0] = mu[:, 0] * htv[:, 0] + mu[:, 1] * htv[:, 1] + D[:, 0] * gv[:, 0] * gt[:, 0] + D[:, 1] * gv[:, 1] * gt[:, 1]
        K[:, 0, 2] = K[:, 2, 0] = mu[:, 2] * htv[:, 2] + mu[:, 3] * htv[:, 3] + D[:, 2] * gv[:, 2] * gt[:, 2] + D[:, 3] * gv[:, 3] * gt[:, 3]
        K[:, 1, 1] = mu[:, 0] * htt[:, 0] + mu[:, 1] * htt[:, 1] + D[:, 0] * gt[:, 0] ** 2 + D[:, 1] * gt[:, 1] ** 2
        K[:, 2, 2] = mu[:, 2] * htt[:, 2] + mu[:, 3] * htt[:, 3] + D[:, 2] * gt[:, 2] ** 2 + D[:, 3] * gt[:, 3] ** 2
    return dict(K=K, D=D, mu=mu, gv=gv, gt=gt, r0=r0, r1=r1, ok=ok, cmax=np.maximum(np.max(cm, axis=1), np.max(cp, axis=1)))


def forward_rhs(c, dd0, dd1):
    """-b_x - S_j D_j alpha_j h_j (n, 3) for the position-delta tangents dd0 = dX0_dot, dd1 = dX1_dot (n,)."""
    q0, q1 = c["r0"] ** 2, c["r1"] ** 2
    al0, al1 = 6 * q0 * dd0, 6 * q1 * dd1
    D, gv, gt, mu = c["D"], c["gv"], c["gt"], c["mu"]
    pa = np.stack([D[:, 0] * al0, -(D[:, 1] * al0), D[:, 2] * al1, -(D[:, 3] * al1)], axis=1)
    rhs = np.zeros((len(dd0), 3))
    rhs[:, 0] = -np.sum(pa * gv, axis=1)
    rhs[:, 1] = -(12 * q0 * c["r0"] * dd0 * (mu[:, 1] - mu[:, 0]) + pa[:, 0] * gt[:, 0] + pa[:, 1] * gt[:, 1])
    rhs[:, 2] = -(12 * q1 * c["r1"] * dd1 * (mu[:, 3] - mu[:, 2]) + pa[:, 2] * gt[:, 2] + pa[:, 3] * gt[:, 3])
    return rhs


# Double-double arithmetic: a value is a pair (hi, lo) of float64 arrays with hi + lo exact, ~106 significant bits.  The error-free
# transformations are the kernels' (two_prod by Dekker's split here, by a fused multiply-add on the device: both exact, so the two
# agree bit for bit away from underflow).
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd(a):
    a = np.asarray(a, dtype=np.float64)
    return a, np.zeros_like(a)


def dd_add(x, y):
    s1, s2 = _two_sum(x[0], y[0])
    t1, t2 = _two_sum(x[1], y[1])
    s1, s2 = _quick(s1, s2 + t1)
    return _quick(s1, s2 + t2)


def dd_neg(x):
    return -x[0], -x[1]


def dd_sub(x, y):
    return dd_add(x, dd_neg(y))


def dd_mul_d(x, c):
    p, e = _two_prod(x[0], c)
    return _quick(p, e + x[1] * c)


def dd_prod(a, b):
    """a * b of two float64 values, exactly"""
    return _two_prod(a, b)


def dd_mul(x, y):
    p, e = _two_prod(x[0], y[0])
    return _quick(p, e + (x[0] * y[1] + x[1] * y[0]))


def dd_div(x, y):
    q1 = x[0] / y[0]
    r = dd_sub(x, dd_mul_d(y, q1))
    return _quick(q1, r[0] / y[0])


def condensed_dd(states, limit=L_DEFAULT):
    """The kernels' K in double-double (dict key "Kdd": K[a][b] = (hi, lo) pairs; "Dgv", "Dgt": the exact products D_j h_j): every
    product of D_j and the pair's gradients formed exactly, so that K carries W below the D_j h_j h_j^T part.  The other keys are
    condensed()'s (K there: the float64 form, the rejected naive form's)."""
    c = condensed(states, limit)
    s = np.asarray(states, dtype=np.float64)
    v, r0, r1 = s[:, 0], c["r0"], c["r1"]
    q0, q1 = r0 * r0, r1 * r1
    u0, u1 = (s[:, 13] - s[:, 11]) * r0, (s[:, 14] - s[:, 13]) * r1
    v0, v2 = s[:, 12], s[:, 15]
    m0, n0 = -4 * v0 - 2 * v, 2 * v0 + 4 * v
    m1, n1 = -4 * v - 2 * v2, 2 * v + 4 * v2
    htt = np.stack([(36 * u0 + 2 * m0) * q0 * r0, (-36 * u0 + 2 * n0) * q0 * r0,
                    (36 * u1 + 2 * m1) * q1 * r1, (-36 * u1 + 2 * n1) * q1 * r1], axis=1)
    htv = np.stack([2 * q0, -4 * q0, 4 * q1, -2 * q1], axis=1)
    D, mu, gv, gt = c["D"], c["mu"], c["gv"], c["gt"]
    with np.errstate(all="ignore"):
        Dgv = [dd_prod(D[:, j], gv[:, j]) for j in range(4)]      # D_j gv_j, exact
        Dgt = [dd_prod(D[:, j], gt[:, j]) for j in range(4)]
        k00 = dd_mul_d(Dgv[0], gv[:, 0])
        for j in range(1, 4):
            k00 = dd_add(k00, dd_mul_d(Dgv[j], gv[:, j]))
        W01 = mu[:, 0] * htv[:, 0] + mu[:, 1] * htv[:, 1]      # W in float64, as the Hessian's 7 x 7 system has it
        W02 = mu[:, 2] * htv[:, 2] + mu[:, 3] * htv[:, 3]
        W11 = mu[:, 0] * htt[:, 0] + mu[:, 1] * htt[:, 1]
        W22 = mu[:, 2] * htt[:, 2] + mu[:, 3] * htt[:, 3]
        k01 = dd_add(dd(W01), dd_add(dd_mul_d(Dgv[0], gt[:, 0]), dd_mul_d(Dgv[1], gt[:, 1])))
        k02 = dd_add(dd(W02), dd_add(dd_mul_d(Dgv[2], gt[:, 2]), dd_mul_d(Dgv[3], gt[:, 3])))
        k11 = dd_add(dd(W11), dd_add(dd_mul_d(Dgt[0], gt[:, 0]), dd_mul_d(Dgt[1], gt[:, 1])))
        k22 = dd_add(dd(W22), dd_add(dd_mul_d(Dgt[2], gt[:, 2]), dd_mul_d(Dgt[3], gt[:, 3])))
    z = dd(np.zeros(len(s)))
    c["Kdd"] = [[k00, k01, k02], [k01, k11, z], [k02, z, k22]]
    c["Dgv"], c["Dgt"] = Dgv, Dgt
    return c


def forward_rhs_dd(c, dd0, dd1):
    """-b_x - S_j D_j alpha_j h_j in double-double: [3] of (hi, lo) pairs, from the exact D_j h_j."""
    q0, q1 = c["r0"] ** 2, c["r1"] ** 2
    al = [6 * q0 * dd0, -(6 * q0 * dd0), 6 * q1 * dd1, -(6 * q1 * dd1)]      # alpha_j
    mu, Dgv, Dgt = c["mu"], c["Dgv"], c["Dgt"]
    with np.errstate(all="ignore"):
        r0 = dd_add(dd_add(dd_mul_d(Dgv[0], al[0]), dd_mul_d(Dgv[1], al[1])), dd_add(dd_mul_d(Dgv[2], al[2]), dd_mul_d(Dgv[3], al[3])))
        r1 = dd_add(dd(12 * q0 * c["r0"] * dd0 * (mu[:, 1] - mu[:, 0])), dd_add(dd_mul_d(Dgt[0], al[0]), dd_mul_d(Dgt[1], al[1])))
        r2 = dd_add(dd(12 * q1 * c["r1"] * dd1 * (mu[:, 3] - mu[:, 2])), dd_add(dd_mul_d(Dgt[2], al[2]), dd_mul_d(Dgt[3], al[3])))
    return [dd_neg(r0), dd_neg(r1), dd_neg(r2)]


def gepp_dd(K, B):
    """X with K X = B for the 3 x 3 double-double K (nested lists of (hi, lo)) and R right-hand sides B ([R][3] of (hi, lo)): the
    kernels' elimination (solve_pivoted's pivot order, compared on the high parts), every operation in double-double."""
    A = [[K[i][k] for k in range(3)] for i in range(3)]
    B = [list(b) for b in B]
    R = len(B)
    with np.errstate(all="ignore"):
        for k in range(2):
            for r in range(k + 1, 3):
                sw = np.abs(A[r][k][0]) > np.abs(A[k][k][0])
                for col in range(k, 3):
                    a, o = A[k][col], A[r][col]
                    A[k][col] = (np.where(sw, o[0], a[0]), np.where(sw, o[1], a[1]))
                    A[r][col] = (np.where(sw, a[0], o[0]), np.where(sw, a[1], o[1]))
                for q in range(R):
                    a, o = B[q][k], B[q][r]
                    B[q][k] = (np.where(sw, o[0], a[0]), np.where(sw, o[1], a[1]))
                    B[q][r] = (np.where(sw, a[0], o[0]), np.where(sw, a[1], o[1]))
            for r in range(k + 1, 3):
                f = dd_div(A[r][k], A[k][k])
                for col in range(k + 1, 3):
                    A[r][col] = dd_sub(A[r][col], dd_mul(f, A[k][col]))
                for q in range(R):
                    B[q][r] = dd_sub(B[q][r], dd_mul(f, B[q][k]))
        X = [[None] * 3 for _ in range(R)]
        for q in range(R):
            for k in range(2, -1, -1):
                acc = B[q][k]
                for col in range(k + 1, 3):
                    acc = dd_sub(acc, dd_mul(A[k][col], X[q][col]))
                X[q][k] = dd_div(acc, A[k][k])
    return X


def _hi(X):
    """(n, R, 3) float64: the rounded solutions"""
    return np.stack([np.stack([x[0] for x in row], axis=1) for row in X], axis=1)


def condensed_vjp(states, g, limit=L_DEFAULT):
    """theta_bar (n, 3) float64 as k_solution_vjp forms it: K w = g in double-double, s_j = D_j h_j . w from the exact D_j h_j."""
    g = np.asarray(g, dtype=np.float64)
    c = condensed_dd(states, limit)
    w = gepp_dd(c["Kdd"], [[dd(g[:, 0]), dd(g[:, 1]), dd(g[:, 2])]])[0]
    with np.errstate(all="ignore"):
        sj = []
        for j in range(4):
            seg = 1 + (j >> 1)
            t = dd_add(dd_mul(c["Dgv"][j], w[0]), dd_mul(c["Dgt"][j], w[seg]))
            sj.append(t[0])
        wx = [x[0] for x in w]
        q0, q1 = c["r0"] ** 2, c["r1"] ** 2
        mu = c["mu"]
        dx0 = -(12 * q0 * c["r0"] * wx[1] * (mu[:, 1] - mu[:, 0]) + 6 * q0 * (sj[0] - sj[1]))
        dx1 = -(12 * q1 * c["r1"] * wx[2] * (mu[:, 3] - mu[:, 2]) + 6 * q1 * (sj[2] - sj[3]))
    out = np.stack([-dx0, dx0 - dx1, dx1], axis=1)
    out[~c["ok"]] = np.nan
    return out


def condensed_jvp(states, tdot, limit=L_DEFAULT):
    """x_dot (n, 3) float64: the condensed forward solve of k_solution_jvp (double-double K and right-hand side); NaN rows for
    non-finite or infeasible states."""
    tdot = np.asarray(tdot, dtype=np.float64)
    c = condensed_dd(states, limit)
    rhs = forward_rhs_dd(c, tdot[:, 1] - tdot[:, 0], tdot[:, 2] - tdot[:, 1])
    out = _hi(gepp_dd(c["Kdd"], [rhs]))[:, 0]
    out[~c["ok"]] = np.nan
    return out


def condensed_jacobian(states, limit=L_DEFAULT):
    """J (n, 3, 3) float64 as k_solution_jacobian forms it: one double-double elimination on the two dX directions."""
    c = condensed_dd(states, limit)
    n = len(c["ok"])
    one, zero = np.ones(n), np.zeros(n)
    d = _hi(gepp_dd(c["Kdd"], [forward_rhs_dd(c, one, zero), forward_rhs_dd(c, zero, one)]))
    d[~c["ok"]] = np.nan
    return np.stack([-d[:, 0], d[:, 0] - d[:, 1], d[:, 1]], axis=2)
