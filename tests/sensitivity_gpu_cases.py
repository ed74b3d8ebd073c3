"""The cases of tests/test_gpu_sensitivity.py, each run in a fresh process (`python tests/sensitivity_gpu_cases.py <case>`): torch
must initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py), which a pytest process that has
already run other GPU tests cannot guarantee.  Not collected by pytest (no test_ prefix on the file)."""
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pytest  # noqa: E402

import rocket_path_amd as rp  # noqa: E402
import sensitivity_ref as sr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from test_sensitivity_cpu import IDENTITY_BOUND  # noqa: E402

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _device_vjp(b, g):
    """theta_bar (n, 3) of Batch b for upstream gradients g (n, 3) host array, or None for zeros."""
    gs = [_t(g[:, k]) for k in range(3)] if g is not None else [None] * 3
    bars = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    b.solution_vjp(*[x.data_ptr() if x is not None else 0 for x in gs], *[x.data_ptr() for x in bars])
    b.sync()
    return np.stack([x.cpu().numpy() for x in bars], axis=1)


def _solved_batch(p, gap_tol=1e-8, max_iter=200):
    b = rp.Batch(len(p[0]), rp.VARIANT_F3, rp.DTYPE_F64, device=0)
    b.set_problems(*p)
    b.solve(gap_tol, max_iter, 0)
    return b


def test_device_vjp_matches_longdouble_restatement():
    oracle = Oracle()
    n = 65536
    p = [np.concatenate(x) for x in zip(rp.problems.generate(31, 0, n // 2, rp.problems.DIST_MONOTONE),
                                        rp.problems.generate(31, 0, n // 2, rp.problems.DIST_REFERENCE_LIKE))]
    with _solved_batch(p) as b:
        states = b.get_state()
        g = np.random.default_rng(5).standard_normal((n, 3))
        dev = _device_vjp(b, g)
    ref = sr.vjp(oracle, states, g).astype(np.float64)
    assert np.all(np.isfinite(dev))
    err = np.linalg.norm(dev - ref, axis=1) / np.linalg.norm(ref, axis=1)
    i = int(np.argmax(err))
    print("device VJP vs longdouble restatement, %d problems: median %.2e, 99.9 %% %.2e, worst %.2e (problem %d)"
          % (n, np.median(err), np.percentile(err, 99.9), err[i], i))
    assert np.percentile(err, 99.9) <= 1e-8 and err.max() <= 1e-5


def test_identities_at_full_size():
    n = 1 << 20
    p = rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)      # bench.py's batch
    with _solved_batch(p) as b:
        states = b.get_state()
        tb = _device_vjp(b, np.random.default_rng(6).standard_normal((n, 3)))
        J = np.stack([_device_vjp(b, np.tile(np.eye(3)[k], (n, 1))) for k in range(3)], axis=1)      # J[:, k, j] = dx_k / dpos_j
    trans = np.abs(tb.sum(axis=1)) / np.max(np.abs(tb), axis=1)
    pos, x = np.stack(p, axis=1), states[:, :3]
    hom = np.max(np.abs(np.einsum("nkj,nj->nk", J, pos) - x / 2), axis=1) / np.max(np.abs(x), axis=1)
    total = J[:, 1] + J[:, 2]
    t0, t1, lam = states[:, 1], states[:, 2], states[:, 3:11]
    mu = lam[:, 1::2] - lam[:, 0::2]
    d0, d1 = 6 / t0**2 * (mu[:, 0] - mu[:, 1]), 6 / t1**2 * (mu[:, 2] - mu[:, 3])      # S lam_i dc_i/d dX
    env = np.max(np.abs(total - np.stack([-d0, d0 - d1, d1], axis=1)), axis=1) / np.max(np.abs(total), axis=1)
    print("1 Mi problems: translation %.2e, homogeneity %.2e, envelope median %.2e / 99.9 %% %.2e / worst %.2e"
          % (trans.max(), hom.max(), np.median(env), np.percentile(env, 99.9), env.max()))
    bound = IDENTITY_BOUND[1e-8]
    assert trans.max() <= 1e-12
    assert hom.max() <= bound["hom"]
    assert np.percentile(env, 99.9) <= bound["env_999"] and env.max() <= bound["env"]


def test_min_time_solve_forward_equals_batch_path_bit_for_bit():
    n = 4096
    p = rp.problems.generate(41, 0, n, rp.problems.DIST_MONOTONE)
    v, d0, d1, it, st = rp.min_time_solve(*[_t(x) for x in p])
    torch.cuda.synchronize()
    with _solved_batch(p) as b:
        rec = torch.empty((n, 4), dtype=torch.float64, device=DEV)
        b.solution_device(rec.data_ptr())
        b.sync()
    rec = rec.cpu().numpy().view(np.dtype(rp.capi.SOLUTION_FIELDS)).reshape(n)
    for name, got in (("vel1", v), ("duration0", d0), ("duration1", d1)):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), rec[name].view(np.uint64)), name
    assert np.array_equal(it.cpu().numpy(), rec["iters"]) and np.array_equal(st.cpu().numpy().view(np.uint32), rec["status"])
    assert it.dtype == torch.int32 and not v.requires_grad


def _vjp_of_state(states, g):
    with rp.Batch(len(states), rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_state(states)
        return _device_vjp(b, g)


def test_vjp_on_pipeline_batch_and_after_nudge_equals_set_state():
    n = 8192
    p = rp.problems.generate(43, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    g = np.random.default_rng(7).standard_normal((n, 3))
    with rp.Pipeline(n, depth=2, n_streams=2) as pl:
        pos = [_t(x) for x in p]
        torch.cuda.synchronize()
        job = pl.submit(*[x.data_ptr() for x in pos])
        pl.wait(job)
        b = pl.batch(job)
        got = _device_vjp(b, g)
        states = b.get_state()
    assert np.all(np.isfinite(got))
    assert np.array_equal(got.view(np.uint64), _vjp_of_state(states, g).view(np.uint64))
    with _solved_batch(p) as b:
        b.nudge(0, 0.25)      # vel1 += 0.25: a state off the central path, still inside
        got = _device_vjp(b, g)
        states = b.get_state()
    assert np.array_equal(got.view(np.uint64), _vjp_of_state(states, g).view(np.uint64))
    # NULL upstream gradients count as zeros
    with _solved_batch(p) as b:
        g0 = g.copy()
        g0[:, 1] = 0
        bars = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(3)]
        gs = [_t(g[:, 0]), None, _t(g[:, 2])]
        b.solution_vjp(*[x.data_ptr() if x is not None else 0 for x in gs], *[x.data_ptr() for x in bars])
        b.sync()
        assert np.array_equal(np.stack([x.cpu().numpy() for x in bars], axis=1), _device_vjp(b, g0))


def test_autograd_total_time_matches_finite_differences():
    n = 4096
    p = rp.problems.generate(47, 0, n, rp.problems.DIST_MONOTONE)
    pos = [_t(x).requires_grad_() for x in p]
    _, d0, d1, _, st = rp.min_time_solve(*pos, gap_tol=1e-13)
    (d0 + d1).sum().backward()
    grad = np.stack([x.grad.cpu().numpy() for x in pos], axis=1)
    outside = (st.cpu().numpy() & (rp.ST_NONFINITE | rp.ST_INFEASIBLE)) != 0      # NaN by definition (include/rp_batch.h)
    assert np.all(np.isfinite(grad[~outside])) and np.all(np.isnan(grad[outside]))

    def solve(q):
        with _solved_batch(q, gap_tol=1e-13) as b:
            return b.get_state()
    base = solve(p)
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1]))
    fd = np.zeros((n, 3))
    ok = ~outside
    for j in range(3):
        lo = [x.copy() for x in p]
        hi = [x.copy() for x in p]
        lo[j] -= h
        hi[j] += h
        s_lo, s_hi = solve(lo), solve(hi)
        fd[:, j] = ((s_hi[:, 1] + s_hi[:, 2]) - (s_lo[:, 1] + s_lo[:, 2])) / (2 * h)
        act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
        ok &= np.all((act(base) == act(s_lo)) & (act(base) == act(s_hi)), axis=1)
    err = np.linalg.norm((grad - fd)[ok], axis=1) / np.linalg.norm(grad[ok], axis=1)
    print("autograd vs finite differences: %d of %d active-set-stable (%d outside the feasible set), worst %.2e"
          % (ok.sum(), n, outside.sum(), err.max()))
    assert ok.mean() > 0.9 and err.max() <= 1e-5


def test_gradient_descent_on_pos1_decreases_total_time():
    n = 1024
    p = rp.problems.generate(53, 0, n, rp.problems.DIST_MONOTONE)
    pos0, pos2 = _t(p[0]), _t(p[2])
    pos1 = _t(p[1]).requires_grad_()
    opt = torch.optim.SGD([pos1], lr=20.0)
    totals = []
    for _ in range(300):
        opt.zero_grad()
        _, d0, d1, _, st = rp.min_time_solve(pos0, pos1, pos2, gap_tol=1e-12)
        total = (d0 + d1).sum()
        total.backward()
        totals.append(total.item())
        opt.step()
    totals = np.array(totals)
    print("gradient descent on pos1: total time %.6f -> %.6f over %d steps" % (totals[0], totals[-1], len(totals)))
    assert np.all(np.diff(totals) < 0)
    assert np.all(st.cpu().numpy() & rp.ST_CONVERGED)


def test_non_monotone_gradients_are_finite():
    # degenerate optimum: 4 active constraints for 3 variables, closed form t_i = sqrt(6 |dX_i| / L)
    n = 4096
    p = rp.problems.generate(59, 0, n, rp.problems.DIST_NON_MONOTONE)
    pos = [_t(x).requires_grad_() for x in p]
    _, d0, d1, _, st = rp.min_time_solve(*pos, gap_tol=1e-10)
    (d0 + d1).sum().backward()
    grad = np.stack([x.grad.cpu().numpy() for x in pos], axis=1)
    assert np.all(np.isfinite(grad))
    dx0, dx1 = p[1] - p[0], p[2] - p[1]
    c0, c1 = np.sign(dx0) * 3 / (100.0 * np.sqrt(6 * np.abs(dx0) / 100.0)), np.sign(dx1) * 3 / (100.0 * np.sqrt(6 * np.abs(dx1) / 100.0))
    closed = np.stack([-c0, c0 - c1, c1], axis=1)
    dist = np.linalg.norm(grad - closed, axis=1) / np.linalg.norm(closed, axis=1)
    print("non-monotone: relative distance to the closed-form derivative: median %.2e, 99 %% %.2e, worst %.2e"
          % (np.median(dist), np.percentile(dist, 99), dist.max()))


def test_unsupported_modes_raise():
    for variant, dtype in ((rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F3, rp.DTYPE_F32), (rp.VARIANT_F3, rp.DTYPE_F32_STATE)):
        with rp.Batch(64, variant, dtype, device=0) as b:
            b.init_default()
            with pytest.raises(rp.RpError) as e:
                b.solution_vjp(0, 0, 0, 0, 0, 0)
            assert e.value.status == rp.capi.RP_ERR_UNSUPPORTED, (variant, dtype)


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
