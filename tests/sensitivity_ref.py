"""Test-side restatement of the solution's sensitivity to the positions, in np.longdouble.

For an F3 state z = (x, lam), x = (vel1, duration0, duration1), and positions theta = (pos0, pos1, pos2):
    M = dr/dz                      the Newton matrix the reference assembles (Oracle.kkt: onedpath_ip.cpp:814-861)
    M^T w = [g; 0_8]               one solve per problem (Gaussian elimination with partial pivoting, batched)
    theta_bar = -w^T dr/dtheta     dr/dtheta analytic: r depends on theta through dX0 = pos1 - pos0, dX1 = pos2 - pos1
Independent of the kernel: the matrix comes from the oracle, the elimination is the textbook one on the full 11 x 11
system, and the arithmetic has 64 mantissa bits.
"""
import numpy as np

LD = np.longdouble
L_DEFAULT = 100.0


def kkt_batch(orc, states):
    """M (n, 11, 11) as float64, from the oracle."""
    return np.stack([orc.kkt(3, s)[0] for s in states])


def drdtheta(states):
    """dr/dtheta (n, 11, 3) in longdouble, analytic (the accelerations are affine in dX0, dX1)."""
    s = np.asarray(states, dtype=LD)
    n = s.shape[0]
    t0, t1 = s[:, 1], s[:, 2]
    lam = s[:, 3:11]
    # d a_j / d dX and d(d a_j / d t_seg) / d dX, j = 0..3 (seg 0 initial, seg 0 final, seg 1 initial, seg 1 final)
    da = np.stack([6 / t0**2, -6 / t0**2, 6 / t1**2, -6 / t1**2], axis=1)
    dgt = np.stack([-12 / t0**3, 12 / t0**3, -12 / t1**3, 12 / t1**3], axis=1)
    d = np.zeros((n, 11, 2), dtype=LD)      # columns: dX0, dX1
    for i in range(8):
        j, sign = i >> 1, (1 if i & 1 else -1)      # even i: -a - L, odd i: a - L
        seg = j >> 1
        d[:, 3 + i, seg] = lam[:, i] * sign * da[:, j]
        d[:, 1 + seg, seg] += lam[:, i] * sign * dgt[:, j]      # the time derivative of constraint i, row duration_seg
    out = np.zeros((n, 11, 3), dtype=LD)
    out[:, :, 0] = -d[:, :, 0]
    out[:, :, 1] = d[:, :, 0] - d[:, :, 1]
    out[:, :, 2] = d[:, :, 1]
    return out


def solve_batched(A, b):
    """x with A x = b for every problem: Gaussian elimination with partial pivoting, vectorised over the batch."""
    A = np.array(A, dtype=LD)
    b = np.array(b, dtype=LD)
    n, m, _ = A.shape
    rows = np.arange(n)
    for k in range(m):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        Ak, Ap = A[rows, k].copy(), A[rows, p].copy()
        A[rows, k], A[rows, p] = Ap, Ak
        bk, bp = b[rows, k].copy(), b[rows, p].copy()
        b[rows, k], b[rows, p] = bp, bk
        f = A[:, k + 1:, k] / A[:, k, k][:, None]
        A[:, k + 1:, :] -= f[:, :, None] * A[:, k, :][:, None, :]
        b[:, k + 1:] -= f * b[:, k][:, None]
    x = np.zeros((n, m), dtype=LD)
    for k in range(m - 1, -1, -1):
        x[:, k] = (b[:, k] - np.sum(A[:, k, k + 1:] * x[:, k + 1:], axis=1)) / A[:, k, k]
    return x


def vjp(orc, states, g):
    """theta_bar (n, 3) longdouble for upstream gradients g (n, 3) on (vel1, duration0, duration1)."""
    M = kkt_batch(orc, states)
    rhs = np.zeros((len(states), 11), dtype=LD)
    rhs[:, :3] = np.asarray(g, dtype=LD)
    w = solve_batched(np.transpose(M, (0, 2, 1)), rhs)
    return -np.einsum("ni,nij->nj", w, drdtheta(states))


def jacobian(orc, states):
    """d(vel1, duration0, duration1) / d(pos0, pos1, pos2): (n, 3, 3), row k = vjp with g = e_k."""
    M = np.transpose(kkt_batch(orc, states), (0, 2, 1))
    D = drdtheta(states)
    n = len(states)
    J = np.zeros((n, 3, 3), dtype=LD)
    for k in range(3):
        rhs = np.zeros((n, 11), dtype=LD)
        rhs[:, k] = 1
        J[:, k, :] = -np.einsum("ni,nij->nj", solve_batched(M, rhs), D)
    return J


def constraint_dtheta(states):
    """d c_i / d theta (n, 8, 3), longdouble (for the envelope identity)."""
    D = drdtheta(states)
    lam = np.asarray(states, dtype=LD)[:, 3:11]
    return D[:, 3:11, :] / lam[:, :, None]


def solved_states(orc, p0, p1, p2, gap_tol, max_iter=200):
    """Oracle-solved F3 states from the feasible start, and the step counts."""
    aos = orc.batch_init_feasible(3, p0, p1, p2)
    it, _ = orc.batch_solve_gated(3, aos, gap_tol, max_iter)
    return aos, it
