"""Test-side restatements of the forward-mode derivative of an F3 solution (rp_batch_solution_jvp, rp_batch_solution_jacobian;
DESIGN.md section 12).

For an F3 state z = (x, lam) and position tangents theta_dot = (pos0_dot, pos1_dot, pos2_dot):
    M z_dot = -(dr/dtheta) theta_dot,    x_dot = z_dot[:3]
full_jvp solves this 11 x 11 system in np.longdouble with M from the oracle (Oracle.kkt) and dr/dtheta from
tests/sensitivity_ref.drdtheta.  condensed_jvp / condensed_jacobian restate the kernels' condensed 3 x 3 form in float64 (the same
K, D_j, mu_j, right-hand side and NaN rule as csrc/sensitivity.hip, each elimination by LAPACK), so the accuracy of the condensation
can be measured on the CPU.
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
    """The kernels' condensed system: dict of K (n, 3, 3), D, mu, gv, gt (n, 4), r0, r1 (n,), ok (n,) -- float64."""
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
    return dict(K=K, D=D, mu=mu, gv=gv, gt=gt, r0=r0, r1=r1, ok=ok)


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


def _solve(K, rhs, ok):
    out = np.full(rhs.shape, np.nan)
    out[ok] = np.linalg.solve(K[ok], rhs[ok])
    return out


def condensed_jvp(states, tdot, limit=L_DEFAULT):
    """x_dot (n, 3) float64: the condensed forward solve of k_solution_jvp; NaN rows for non-finite or infeasible states."""
    tdot = np.asarray(tdot, dtype=np.float64)
    c = condensed(states, limit)
    with np.errstate(all="ignore"):
        rhs = forward_rhs(c, tdot[:, 1] - tdot[:, 0], tdot[:, 2] - tdot[:, 1])
    return _solve(c["K"], rhs[..., None], c["ok"])[..., 0]


def condensed_jacobian(states, limit=L_DEFAULT):
    """J (n, 3, 3) float64 as k_solution_jacobian forms it: one elimination on the two dX directions."""
    c = condensed(states, limit)
    n = len(c["ok"])
    one, zero = np.ones(n), np.zeros(n)
    with np.errstate(all="ignore"):
        rhs = np.stack([forward_rhs(c, one, zero), forward_rhs(c, zero, one)], axis=2)
    d = _solve(c["K"], rhs, c["ok"])
    return np.stack([-d[:, :, 0], d[:, :, 0] - d[:, :, 1], d[:, :, 1]], axis=2)
