"""Test-side restatements for problems with end velocities (rp_batch_set_problems_vel_device, rp_batch_solution_*_vel; DESIGN.md
section 12).

start_state restates the start rule in numpy.  For theta = (pos0, pos1, pos2, vel0, vel2):
    drdtheta5       dr/dtheta (n, 11, 5) in longdouble, analytic: the position columns of tests/sensitivity_ref.drdtheta and the two
                    velocity columns (d a / d vel0 = (-4, 2) / t0, d (d a / d t0) / d vel0 = (4, -2) / t0^2; vel2: (-2, 4) / t1 and
                    (2, -4) / t1^2), checked against central differences of residual_ld by the CPU tests
    full_jacobian5  J = -M^-1 dr/dtheta (n, 3, 5) on the full 11 x 11 system in longdouble (M = kkt_ld)
    condensed_*5    the kernels' condensed double-double arithmetic (csrc/sensitivity.hip, the k_endvel_* kernels) restated with the helpers of
                    tests/sensitivity_jvp_ref.py
"""
import numpy as np

import sensitivity_hess_ref as hr
import sensitivity_jvp_ref as jr
import sensitivity_ref as sr

LD = np.longdouble
L_DEFAULT = 100.0


def start_state(p0, p1, p2, v0, v2, limit=L_DEFAULT, variant=3, storage=np.float64):
    """The start of rp_batch_set_problems_vel(_device) in the reference's AoS layout (n, 16 or 12), from the values as stored
    (`storage`: the batch's field type): vel1 0, multipliers 1, t_i = (3.5/sqrt 12) sqrt(6 |dX_i| / L) + 8 |vel_end| / L."""
    m = 8 if variant == 3 else 4
    cb = 3 + m
    s0, s1, s2, w0, w2 = (np.asarray(a, dtype=np.float64).astype(storage).astype(np.float64) for a in (p0, p1, p2, v0, v2))
    w0, w2 = w0 + 0.0, w2 + 0.0      # -0 is stored as +0
    scale = 3.5 / np.sqrt(12.0)
    st = np.zeros((len(s0), cb + 5))
    st[:, 1] = (scale * np.sqrt(6.0 * np.abs(s1 - s0) / limit) + 8.0 * np.abs(w0) / limit).astype(storage)
    st[:, 2] = (scale * np.sqrt(6.0 * np.abs(s2 - s1) / limit) + 8.0 * np.abs(w2) / limit).astype(storage)
    st[:, 3:cb] = 1.0
    st[:, cb + 0], st[:, cb + 1], st[:, cb + 2], st[:, cb + 3], st[:, cb + 4] = s0, w0, s1, s2, w2
    return st


def velocities(orc, dist, kappa, n, seed):
    """Problems of generator `dist` and end velocities kappa U(-1, 1) sqrt(L |dX|) of their own segment: (p0, p1, p2, v0, v2)."""
    p0, p1, p2 = orc.gen_problems(seed, 0, n, dist)
    rng = np.random.default_rng(seed)
    v0 = kappa * rng.uniform(-1, 1, n) * np.sqrt(L_DEFAULT * np.abs(p1 - p0))
    v2 = kappa * rng.uniform(-1, 1, n) * np.sqrt(L_DEFAULT * np.abs(p2 - p1))
    return p0, p1, p2, v0, v2


def family(orc, dist, kappa, gap_tol, n=1024, seed=31, max_iter=200):
    """(inputs, start, oracle-solved states, step counts) of the velocity family."""
    args = velocities(orc, dist, kappa, n, seed)
    start = start_state(*args)
    st = start.copy()
    it, _ = orc.batch_solve_gated(3, st, gap_tol, max_iter)
    return args, start, st, it


def drdtheta5(states):
    """dr/dtheta (n, 11, 5) in longdouble, columns (pos0, pos1, pos2, vel0, vel2)."""
    s = np.asarray(states, dtype=LD)
    n = len(s)
    t0, t1 = s[:, 1], s[:, 2]
    lam = s[:, 3:11]
    da = np.stack([-4 / t0, 2 / t0, -2 / t1, 4 / t1], axis=1)                   # d a_j / d vel_end of its segment
    dgt = np.stack([4 / t0**2, -2 / t0**2, 2 / t1**2, -4 / t1**2], axis=1)      # d (d a_j / d t_seg) / d vel_end
    d = np.zeros((n, 11, 2), dtype=LD)
    for i in range(8):
        j, sign = i >> 1, (1 if i & 1 else -1)
        seg = j >> 1
        d[:, 3 + i, seg] = lam[:, i] * sign * da[:, j]
        d[:, 1 + seg, seg] += lam[:, i] * sign * dgt[:, j]
    return np.concatenate([sr.drdtheta(states), d], axis=2)


def full_jacobian5(states, limit=L_DEFAULT):
    """d(vel1, duration0, duration1) / d theta (n, 3, 5) longdouble: the 11 x 11 system, every column solved."""
    M = hr.kkt_ld(states, limit)
    D = drdtheta5(states)
    return np.stack([sr.solve_batched(M, -D[:, :, b])[:, :3] for b in range(5)], axis=2)


def _rhs5_dd(c, dd0, dd1, e0, e2):
    """forward_rhs<true> of csrc/sensitivity_core.h in double-double."""
    r0, r1 = c["r0"], c["r1"]
    q0, q1 = r0 ** 2, r1 ** 2
    al = [6 * q0 * dd0 + -4.0 * r0 * e0, -(6 * q0 * dd0) + 2.0 * r0 * e0, 6 * q1 * dd1 + -2.0 * r1 * e2, -(6 * q1 * dd1) + 4.0 * r1 * e2]
    mu, Dgv, Dgt = c["mu"], c["Dgv"], c["Dgt"]
    with np.errstate(all="ignore"):
        x0 = jr.dd_add(jr.dd_add(jr.dd_mul_d(Dgv[0], al[0]), jr.dd_mul_d(Dgv[1], al[1])),
                       jr.dd_add(jr.dd_mul_d(Dgv[2], al[2]), jr.dd_mul_d(Dgv[3], al[3])))
        x1 = jr.dd_add(jr.dd(12 * q0 * r0 * dd0 * (mu[:, 1] - mu[:, 0]) + q0 * e0 * (4.0 * mu[:, 0] - 2.0 * mu[:, 1])),
                       jr.dd_add(jr.dd_mul_d(Dgt[0], al[0]), jr.dd_mul_d(Dgt[1], al[1])))
        x2 = jr.dd_add(jr.dd(12 * q1 * r1 * dd1 * (mu[:, 3] - mu[:, 2]) + q1 * e2 * (2.0 * mu[:, 2] - 4.0 * mu[:, 3])),
                       jr.dd_add(jr.dd_mul_d(Dgt[2], al[2]), jr.dd_mul_d(Dgt[3], al[3])))
    return [jr.dd_neg(x0), jr.dd_neg(x1), jr.dd_neg(x2)]


def _ok(states, c):
    s = np.asarray(states, dtype=np.float64)
    return c["ok"] & (s[:, 1] > 0) & (s[:, 2] > 0)


def condensed_vjp5(states, g, limit=L_DEFAULT):
    """theta_bar (n, 5) float64 as k_endvel_vjp forms it."""
    g = np.asarray(g, dtype=np.float64)
    c = jr.condensed_dd(states, limit)
    w = jr.gepp_dd(c["Kdd"], [[jr.dd(g[:, 0]), jr.dd(g[:, 1]), jr.dd(g[:, 2])]])[0]
    with np.errstate(all="ignore"):
        sj = [jr.dd_add(jr.dd_mul(c["Dgv"][j], w[0]), jr.dd_mul(c["Dgt"][j], w[1 + (j >> 1)]))[0] for j in range(4)]
        wx = [x[0] for x in w]
        r0, r1 = c["r0"], c["r1"]
        q0, q1 = r0 ** 2, r1 ** 2
        mu = c["mu"]
        dx0 = -(12 * q0 * r0 * wx[1] * (mu[:, 1] - mu[:, 0]) + 6 * q0 * (sj[0] - sj[1]))
        dx1 = -(12 * q1 * r1 * wx[2] * (mu[:, 3] - mu[:, 2]) + 6 * q1 * (sj[2] - sj[3]))
        v0 = -(q0 * wx[1] * (4.0 * mu[:, 0] - 2.0 * mu[:, 1]) + r0 * (2.0 * sj[1] - 4.0 * sj[0]))
        v2 = -(q1 * wx[2] * (2.0 * mu[:, 2] - 4.0 * mu[:, 3]) + r1 * (4.0 * sj[3] - 2.0 * sj[2]))
    out = np.stack([-dx0, dx0 - dx1, dx1, v0, v2], axis=1)
    out[~_ok(states, c)] = np.nan
    return out


def condensed_jvp5(states, tdot, limit=L_DEFAULT):
    """x_dot (n, 3) float64 as k_endvel_jvp forms it, for tangents tdot (n, 5)."""
    tdot = np.asarray(tdot, dtype=np.float64)
    c = jr.condensed_dd(states, limit)
    rhs = _rhs5_dd(c, tdot[:, 1] - tdot[:, 0], tdot[:, 2] - tdot[:, 1], tdot[:, 3], tdot[:, 4])
    out = jr._hi(jr.gepp_dd(c["Kdd"], [rhs]))[:, 0]
    out[~_ok(states, c)] = np.nan
    return out


def condensed_jacobian5(states, limit=L_DEFAULT):
    """J (n, 3, 5) float64 as k_endvel_jacobian forms it (the elimination's results per right-hand side are solve3_dd's)."""
    c = jr.condensed_dd(states, limit)
    n = len(c["ok"])
    one, zero = np.ones(n), np.zeros(n)
    d = jr._hi(jr.gepp_dd(c["Kdd"], [jr.forward_rhs_dd(c, one, zero), jr.forward_rhs_dd(c, zero, one),
                                      _rhs5_dd(c, zero, zero, one, zero), _rhs5_dd(c, zero, zero, zero, one)]))
    d[~_ok(states, c)] = np.nan
    return np.stack([-d[:, 0], d[:, 0] - d[:, 1], d[:, 1], d[:, 2], d[:, 3]], axis=2)


def rel(a, b):
    """normwise relative error per problem"""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
