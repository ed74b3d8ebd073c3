"""The cases of tests/test_gpu_sensitivity_edges.py, each run in a fresh process (`python tests/sensitivity_edges_gpu_cases.py <case>`):
the four derivative entries (rp_batch_solution_vjp, _jvp, _jacobian, _hessian) on states away from the default problems -- non-zero
end velocities set through set_state, nudge and field_ptr, other acceleration limits, unsolved states, edge multipliers, and batch
sizes around the 256-lane block in both problem orders -- against the longdouble solve of the full 11 x 11 system
(tests/sensitivity_hess_ref.py).  Not collected by pytest (no test_ prefix on the file)."""
import ctypes
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hip_util  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import sensitivity_hess_ref as hr  # noqa: E402
import sensitivity_jvp_ref as jr  # noqa: E402
from test_sensitivity_edges_cpu import EDGE_BOUND, edge_state, end_velocity_bound  # noqa: E402

DEV = "cuda:0"
N = 65536
DISTS = (rp.problems.DIST_MONOTONE, rp.problems.DIST_REFERENCE_LIKE, rp.problems.DIST_NON_MONOTONE)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mixed(seed, n):
    """n problems: a third each of the monotone, reference-like and non-monotone distributions, and the distribution of each."""
    sizes = [n - 2 * (n // 3), n // 3, n // 3]
    parts = [rp.problems.generate(seed, 0, k, d) for k, d in zip(sizes, DISTS)]
    return [np.concatenate(x) for x in zip(*parts)], np.repeat([0, 1, 2], sizes)


def _derivs(b, g, td):
    """(VJP (n, 3), JVP (n, 3), Jacobian (n, 3, 3), Hessian (n, 3, 3, 3), the Hessian entry's Jacobian) of Batch b, problem order."""
    n = b.n
    gs, ts = [_t(g[:, k]) for k in range(3)], [_t(td[:, k]) for k in range(3)]
    bars = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(3)]
    dots = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(3)]
    jac, jac2 = (torch.empty((n, 3, 3), dtype=torch.float64, device=DEV) for _ in range(2))
    hess = torch.empty((n, 3, 3, 3), dtype=torch.float64, device=DEV)
    b.solution_vjp(*[x.data_ptr() for x in gs], *[x.data_ptr() for x in bars])
    b.solution_jvp(*[x.data_ptr() for x in ts], *[x.data_ptr() for x in dots])
    b.solution_jacobian(jac.data_ptr())
    b.solution_hessian(jac2.data_ptr(), hess.data_ptr())
    b.sync()
    return (np.stack([x.cpu().numpy() for x in bars], axis=1), np.stack([x.cpu().numpy() for x in dots], axis=1),
            jac.cpu().numpy(), hess.cpu().numpy(), jac2.cpu().numpy())


def _rel(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _check(b, limit, label, bound_j, bound_h, seed=0, max_nan=0):
    """Every entry at Batch b's states against the longdouble solve built on kkt_ld(states, limit); translation and exact
    symmetry.  NaN rows only where the kernels' NaN rule puts them (at most max_nan of them: rounding-level c_i > 0 of an active
    constraint).  Returns the states."""
    states = b.get_state()
    n = len(states)
    rng = np.random.default_rng(seed)
    g, td = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    vjp, jvp, J, H, J2 = _derivs(b, g, td)
    ok = np.all(np.isfinite(J.reshape(n, -1)), axis=1)
    for x in (vjp, jvp, H, J2):
        assert np.array_equal(np.all(np.isfinite(x.reshape(n, -1)), axis=1), ok), label
    # the host restatement of the NaN rule agrees but where the largest c_i is within rounding of 0 (fused and unfused
    # arithmetic can put it on either side)
    c = jr.condensed(states, limit)
    assert np.all((ok == c["ok"]) | (np.abs(c["cmax"]) <= 64 * np.finfo(np.float64).eps * limit)), label
    assert (~ok).sum() <= max_nan, (label, int((~ok).sum()))
    s = states[ok]
    Jf, Hf = hr.full_hessian(s, M=hr.kkt_ld(s, limit), limit=limit)
    Jf, Hf = Jf.astype(np.float64), Hf.astype(np.float64)
    e_vjp = _rel(vjp[ok], np.einsum("na,nab->nb", g[ok], Jf))
    e_jvp = _rel(jvp[ok], np.einsum("nab,nb->na", Jf, td[ok]))
    e_j, e_j2, e_h = _rel(J[ok], Jf), _rel(J2[ok], Jf), _rel(H[ok], Hf)
    print("%s: %d rows (%d NaN by the rule); worst VJP %.2e JVP %.2e Jacobian %.2e / %.2e Hessian %.2e (99.9 %% %.2e)"
          % (label, n, (~ok).sum(), e_vjp.max(), e_jvp.max(), e_j.max(), e_j2.max(), e_h.max(), np.percentile(e_h, 99.9)))
    assert max(e_vjp.max(), e_jvp.max(), e_j.max(), e_j2.max()) <= bound_j, label
    assert e_h.max() <= bound_h, label
    Hk = H[ok]
    assert np.array_equal(_bits(Hk), _bits(np.swapaxes(Hk, 2, 3))), label
    tr_j = np.max(np.abs(J[ok].sum(axis=2)), axis=1) / np.max(np.abs(J[ok]), axis=(1, 2))
    tr_h = np.max(np.abs(Hk.sum(axis=3)), axis=(1, 2)) / np.max(np.abs(Hk), axis=(1, 2, 3))
    assert tr_j.max() <= 1e-14 and tr_h.max() <= 1e-14, (label, tr_j.max(), tr_h.max())
    return states


def _end_velocities(st, s, seed):
    rng = np.random.default_rng(seed)
    return s * rng.uniform(-1, 1, len(st)) * st[:, 1], s * rng.uniform(-1, 1, len(st)) * st[:, 2]


def _assert_converged(b, label):
    # with end velocities ~2-3 % of the problems take more than 200 steps to gap 1e-13 (RP_ST_MAXITER): their states get checked too
    it, status = b.get_iters()
    assert np.mean(status == rp.capi.ST_CONVERGED) >= 0.95, (label, np.unique(status, return_counts=True))


def test_end_velocities_through_set_state():
    p, _ = _mixed(71, N)
    for gap in (1e-8, 1e-13):
        for s in (0.02, 0.1):
            with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
                b.set_problems(*p)
                st = b.get_state()
                st[:, 12], st[:, 15] = _end_velocities(st, s, 5)
                b.set_state(st)
                b.solve(gap, 200, 0)
                _assert_converged(b, "set_state")
                bj, bh = end_velocity_bound(gap)
                _check(b, 100.0, "set_state s %g gap %g" % (s, gap), bj, bh, max_nan=N // 2000)


def test_end_velocities_through_nudge():
    p, _ = _mixed(72, N)
    for gap in (1e-8, 1e-13):
        with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems(*p)
            b.nudge(12, 0.05)      # the special keys' vel0 / vel2 moves: the same delta for every problem
            b.nudge(15, -0.03)
            b.solve(gap, 200, 0)
            _assert_converged(b, "nudge")
            states = _check(b, 100.0, "nudge gap %g" % gap, *end_velocity_bound(gap), max_nan=N // 2000)
            assert np.all(states[:, 12] == 0.05) and np.all(states[:, 15] == -0.03)


def test_end_velocities_through_field_ptr():
    p, _ = _mixed(73, N)
    hip = hip_util._hip()
    for gap in (1e-8, 1e-13):
        with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems(*p)
            st = b.get_state()      # writes the start out: the field pointers are defined from here on
            v0, v2 = _end_velocities(st, 0.05, 6)
            slot = b.slot_map()
            for field, vals in ((12, v0), (15, v2)):
                arr = np.empty(N)
                arr[slot] = vals      # batch order
                assert hip.hipMemcpy(ctypes.c_void_p(b.field_ptr(field)), ctypes.c_void_p(arr.ctypes.data), ctypes.c_size_t(arr.nbytes), 1) == 0
            b.solve(gap, 200, 0)
            _assert_converged(b, "field_ptr")
            states = _check(b, 100.0, "field_ptr gap %g" % gap, *end_velocity_bound(gap), max_nan=N // 2000)
            assert np.array_equal(states[:, 12], v0) and np.array_equal(states[:, 15], v2)


def test_other_limits():
    n = 16384
    p, _ = _mixed(74, n)
    for limit in (37.5, 250.0):
        for gap in (1e-8, 1e-13):
            with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
                b.set_params(accel_limit=limit)
                b.set_problems(*p)
                b.solve(gap, 200, 0)
                _assert_converged(b, "limit")
                _check(b, limit, "limit %g gap %g" % (limit, gap), *EDGE_BOUND["default"])
        # autograd at that limit against central differences of the device solve at that limit
        m = 2048
        q = [x[:m] for x in p]
        pos = [_t(x).requires_grad_() for x in q]
        out = rp.min_time_solve(*pos, gap_tol=1e-13, params={"accel_limit": limit})
        with rp.Batch(m, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_params(accel_limit=limit)
            b.set_problems(*q)
            b.solve(1e-13, 200, 0)
            ref = b.get_state()[:, :3]
        assert np.array_equal(_bits(torch.stack(out[:3], 1).detach().cpu().numpy()), _bits(ref))
        wts = np.random.default_rng(9).standard_normal((m, 3))
        loss = sum((out[k] * _t(wts[:, k])).sum() for k in range(3))
        grads = np.stack([x.cpu().numpy() for x in torch.autograd.grad(loss, pos)], axis=1)
        h = 1e-4 * np.maximum(np.abs(q[1] - q[0]), np.abs(q[2] - q[1]))
        fd = np.zeros((m, 3))
        act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
        stable = np.ones(m, dtype=bool)
        with rp.Batch(m, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_params(accel_limit=limit)
            b.set_problems(*q)
            b.solve(1e-13, 200, 0)
            base = b.get_state()
            for k in range(3):
                sides = []
                for sgn in (1, -1):
                    qq = [x.copy() for x in q]
                    qq[k] = qq[k] + sgn * h
                    b.set_problems(*qq)
                    b.solve(1e-13, 200, 0)
                    sides.append(b.get_state())
                    stable &= np.all(act(sides[-1]) == act(base), axis=1)
                fd[:, k] = np.sum(wts * (sides[0][:, :3] - sides[1][:, :3]), axis=1) / (2 * h)
        err = np.abs(grads - fd)[stable] / np.max(np.abs(grads[stable]), axis=1)[:, None]
        print("limit %g: autograd vs differences of the device solve, %d of %d active-set-stable, worst %.2e"
              % (limit, stable.sum(), m, err.max()))
        assert stable.mean() > 0.9 and err.max() <= 1e-5


def test_unsolved_states():
    n = 16384
    p, _ = _mixed(75, n)
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_problems(*p)
        b.get_state()
        _check(b, 100.0, "feasible start", *EDGE_BOUND["unsolved"])
        done = 0
        for k in (1, 3, 8):
            b.step(k - done)
            done = k
            _check(b, 100.0, "%d fixed steps" % k, *EDGE_BOUND["unsolved"])
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_problems(*p)
        b.solve(1e-8, 3, 0)
        it, status = b.get_iters()
        assert np.mean((status & rp.capi.ST_MAXITER) != 0) > 0.9
        _check(b, 100.0, "RP_ST_MAXITER (max_iter 3)", *EDGE_BOUND["unsolved"])
    for init in ("init_default", "init_stuck"):
        with rp.Batch(64, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            getattr(b, init)()
            _check(b, 100.0, init, *EDGE_BOUND["init"])
            b.step(5)
            _check(b, 100.0, init + " + 5 steps", *EDGE_BOUND["init"])


def test_edge_multipliers_and_the_nan_rule():
    n = 4096
    for pair, lam in ((0, 0.0), (1, 1e-170), (2, 0.0), (3, 1e-170)):
        st = edge_state(n, pair, lam, seed=pair)
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_state(st)
            _check(b, 100.0, "pair %d multipliers %g" % (pair, lam), *EDGE_BOUND["edge"])
    # the NaN rule is unchanged: a non-finite field or some c_i > 0 gives NaN rows, the others are untouched
    st = edge_state(n, 0, 0.0, seed=7)
    st[1::4, 5] = np.nan
    st[2::4, 0] = 1e3      # vel1 far outside: infeasible
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_state(st)
        _, _, J, H, _ = _derivs(b, np.ones((n, 3)), np.ones((n, 3)))
    bad = np.zeros(n, dtype=bool)
    bad[1::4] = bad[2::4] = True
    assert np.array_equal(np.all(np.isnan(J.reshape(n, -1)), axis=1), bad)
    assert np.array_equal(np.all(np.isnan(H.reshape(n, -1)), axis=1), bad)
    assert np.all(np.isfinite(H[~bad]))


def _padded_derivs(b, g, td, null_g=()):
    """_derivs with every output inside a sentinel-filled buffer, PAD elements on each side; asserts the padding untouched."""
    n, pad, sentinel = b.n, 37, 0x7FF4DEADBEEF0001
    gs = [None if k in null_g else _t(g[:, k]) for k in range(3)]
    ts = [_t(td[:, k]) for k in range(3)]

    def buf(width):
        return torch.full(((n + 2 * pad) * width,), sentinel, dtype=torch.int64, device=DEV)
    bars, dots = [buf(1) for _ in range(3)], [buf(1) for _ in range(3)]
    jac, jac2, hess = buf(9), buf(9), buf(27)
    at = lambda x, width: x.data_ptr() + 8 * pad * width      # noqa: E731
    b.solution_vjp(*[x.data_ptr() if x is not None else 0 for x in gs], *[at(x, 1) for x in bars])
    b.solution_jvp(*[x.data_ptr() for x in ts], *[at(x, 1) for x in dots])
    b.solution_jacobian(at(jac, 9))
    b.solution_hessian(at(jac2, 9), at(hess, 27))
    b.sync()
    out = []
    for x, width in [(x, 1) for x in bars] + [(x, 1) for x in dots] + [(jac, 9), (hess, 27), (jac2, 9)]:
        a = x.cpu().numpy()
        assert np.all(a[:pad * width] == sentinel) and np.all(a[(n + pad) * width:] == sentinel)
        out.append(a[pad * width:(n + pad) * width].view(np.float64))
    return (np.stack(out[0:3], axis=1), np.stack(out[3:6], axis=1), out[6].reshape(n, 3, 3), out[7].reshape(n, 3, 3, 3),
            out[8].reshape(n, 3, 3))


def test_batch_shapes_and_padding():
    # every lane is independent: a problem's outputs are the same bits in a batch of any size, in either order
    p, _ = _mixed(76, N)
    rng = np.random.default_rng(10)
    g, td = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_problems(*p)
        b.solve(1e-8, 200, 0)
        filler = b.get_state()
    for n in (1, 63, 64, 65, 255, 257, 4097):
        for order in ("scheduled", "set_state"):
            with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
                if order == "scheduled":      # a gated solve: the batch keeps its problems in its own order (prob_of)
                    b.set_problems(*[x[N - n:] for x in p])
                    b.solve(1e-8, 200, 0)
                else:                         # set_state: problem order, prob_of NULL
                    b.set_state(filler[N - n:])
                states = b.get_state()
                got = _padded_derivs(b, g[:n], td[:n])
                for null in ((0,), (1, 2), (0, 1, 2)):
                    gz = g[:n].copy()
                    gz[:, list(null)] = 0.0
                    a = _padded_derivs(b, g[:n], td[:n], null_g=null)[0]
                    r = _padded_derivs(b, gz, td[:n])[0]
                    assert np.array_equal(_bits(a), _bits(r)), (n, order, null)
            big_states = filler.copy()
            big_states[:n] = states
            with rp.Batch(N, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
                b.set_state(big_states)
                big = _padded_derivs(b, g, td)
            for a, r in zip(got, big):
                assert np.array_equal(_bits(a), _bits(r[:n])), (n, order)
            assert np.all(np.isfinite(got[3])), (n, order)
    print("batch shapes: every entry bit for bit the 65,536-problem batch's rows, padding untouched, NULL upstreams = zeros")


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
