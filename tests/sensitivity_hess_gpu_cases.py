"""The cases of tests/test_gpu_sensitivity_hess.py, each run in a fresh process (`python tests/sensitivity_hess_gpu_cases.py <case>`):
torch must initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py).  Not collected by pytest (no
test_ prefix on the file)."""
import gc
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pytest  # noqa: E402

import rocket_path_amd as rp  # noqa: E402
import sensitivity_hess_ref as hr  # noqa: E402
import sensitivity_jvp_gpu_cases as jc  # noqa: E402
import sensitivity_jvp_ref as jr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import autograd  # noqa: E402

DEV = jc.DEV
_t, _bits, _rel = jc._t, jc._bits, jc._rel


def _device_hessian(b, with_jac=True):
    """(J (n, 3, 3) or None, H (n, 3, 3, 3)) of Batch b from one rp_batch_solution_hessian launch."""
    hess = torch.empty((b.n, 3, 3, 3), dtype=torch.float64, device=DEV)
    jac = torch.empty((b.n, 3, 3), dtype=torch.float64, device=DEV) if with_jac else None
    b.solution_hessian(jac.data_ptr() if with_jac else 0, hess.data_ptr())
    b.sync()
    return (jac.cpu().numpy() if with_jac else None), hess.cpu().numpy()


def _flat_rel(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def test_device_hessian_matches_longdouble_restatement():
    oracle = Oracle()
    n = 65536
    p, dist = jc._mixed(103, n)
    with jc._solved_batch(p) as b:
        states = b.get_state()
        J, H = _device_hessian(b)
    Jf, Hf = hr.full_hessian(states, orc=oracle)
    Hf = Hf.astype(np.float64)
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(J))
    err = _flat_rel(H, Hf)
    for d in range(3):
        e = err[dist == d]
        print("dist %d, %d problems: device Hessian vs longdouble median %.2e, 99.9 %% %.2e, worst %.2e"
              % (d, e.size, np.median(e), np.percentile(e, 99.9), e.max()))
    # The tail of the monotone / reference-like problems is the problems' own conditioning, not the kernel's: measured 3.1e-10 worst
    # on one monotone problem with three active constraints (K ~ 1e10), where the longdouble solve itself moves by 2e-10 between
    # the oracle's float64 M and one formed in longdouble from the same state; the float64 restatement shows the same 6e-10 there.
    regular = err[dist < 2]
    assert np.median(regular) <= 1e-14 and np.percentile(regular, 99.9) <= 1e-13 and regular.max() <= 1e-8
    assert err[dist == 2].max() <= 1e-11
    # exact symmetry in (b, c), translation to rounding
    assert np.array_equal(_bits(H), _bits(np.swapaxes(H, 2, 3)))
    scale = np.max(np.abs(H), axis=(1, 2, 3))
    tr = np.max(np.abs(H.sum(axis=3)), axis=(1, 2)) / scale
    print("translation: worst row sum %.2e" % tr.max())
    assert tr.max() <= 1e-12


def test_jacobian_output_and_null_jacobian():
    n = 65536
    p, dist = jc._mixed(107, n)
    with jc._solved_batch(p) as b:
        J, H = _device_hessian(b)
        _, H_nojac = _device_hessian(b, with_jac=False)
        Jk = jc._device_jacobian(b)
    err = np.linalg.norm(J - Jk, axis=(1, 2)) / np.linalg.norm(Jk, axis=(1, 2))
    print("d_jac vs rp_batch_solution_jacobian: worst %.2e (monotone, reference-like), %.2e (non-monotone)"
          % (err[dist < 2].max(), err[dist == 2].max()))
    assert np.all(np.isfinite(J)) and err[dist < 2].max() <= 1e-13 and err[dist == 2].max() <= 1e-12
    assert np.array_equal(_bits(H), _bits(H_nojac))


def test_hessian_matches_differences_of_the_device_jacobian():
    # central differences of rp_batch_solution_jacobian at re-solved positions, on problems whose active set is stable at +-h
    n = 4096
    p = rp.problems.generate(109, 0, n, rp.problems.DIST_MONOTONE)
    rng = np.random.default_rng(21)
    u = rng.standard_normal((n, 3))
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1])) / np.max(np.abs(u), axis=1)

    def at(q):
        with jc._solved_batch(q, gap_tol=1e-13) as b:
            return b.get_state(), jc._device_jacobian(b)
    with jc._solved_batch(p, gap_tol=1e-13) as b:
        base = b.get_state()
        _, H = _device_hessian(b)
    lo, J_lo = at([x - h * u[:, k] for k, x in enumerate(p)])
    hi, J_hi = at([x + h * u[:, k] for k, x in enumerate(p)])
    fd = (J_hi - J_lo) / (2 * h[:, None, None])
    Hu = np.einsum("nabc,nc->nab", H, u)
    act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
    ok = np.all((act(base) == act(lo)) & (act(base) == act(hi)), axis=1)
    err = np.linalg.norm((Hu - fd)[ok], axis=(1, 2)) / np.linalg.norm(Hu[ok], axis=(1, 2))
    print("H u vs differences of the device Jacobian: %d of %d active-set-stable, median %.2e, 99 %% %.2e, worst %.2e"
          % (ok.sum(), n, np.median(err), np.percentile(err, 99), err.max()))
    assert ok.mean() > 0.9 and np.percentile(err, 99) <= 1e-4 and err.max() <= 1e-2


def _of_state(states):
    with rp.Batch(len(states), rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_state(states)
        return _device_hessian(b)


def test_problem_order_on_pipeline_batch_and_after_nudge_equals_set_state():
    n = 8192
    p = rp.problems.generate(113, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    with rp.Pipeline(n, depth=2, n_streams=2) as pl:
        pos = [_t(x) for x in p]
        torch.cuda.synchronize()
        job = pl.submit(*[x.data_ptr() for x in pos])
        pl.wait(job)
        b = pl.batch(job)
        got = _device_hessian(b)
        states = b.get_state()
    assert np.all(np.isfinite(got[1]))
    for a, r in zip(got, _of_state(states)):
        assert np.array_equal(_bits(a), _bits(r))
    with jc._solved_batch(p) as b:
        b.nudge(0, 0.25)      # vel1 moved: a state off the central path
        got = _device_hessian(b)
        states = b.get_state()
    ok = jr.condensed(states)["ok"]      # NaN exactly where the moved state is outside the feasible set
    assert np.array_equal(np.all(np.isfinite(got[1]), axis=(1, 2, 3)), ok)
    for a, r in zip(got, _of_state(states)):
        assert np.array_equal(_bits(a), _bits(r))


def test_nan_rows_and_unsupported_modes():
    n = 4096
    p = rp.problems.generate(127, 0, n, rp.problems.DIST_MONOTONE)
    with jc._solved_batch(p) as b:
        states = b.get_state()
    bad_inf = np.arange(0, n, 7)
    bad_nan = np.arange(3, n, 11)
    states[bad_inf, 1] *= 0.1      # duration0 / 10: accelerations x 100, outside |a| <= L
    states[bad_nan, 5] = np.nan
    bad = np.zeros(n, dtype=bool)
    bad[bad_inf] = bad[bad_nan] = True
    J, H = _of_state(states)
    assert np.all(np.isnan(H[bad])) and np.all(np.isfinite(H[~bad]))
    assert np.all(np.isnan(J[bad])) and np.all(np.isfinite(J[~bad]))
    for variant, dtype in ((rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F3, rp.DTYPE_F32), (rp.VARIANT_F3, rp.DTYPE_F32_STATE)):
        with rp.Batch(64, variant, dtype, device=0) as b:
            b.init_default()
            with pytest.raises(rp.RpError) as e:
                b.solution_hessian(0, 0)
            assert e.value.status == rp.capi.RP_ERR_UNSUPPORTED, (variant, dtype)
    with rp.Batch(64, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.init_default()
        with pytest.raises(rp.RpError) as e:
            b.solution_hessian(0, 0)
        assert e.value.status == rp.capi.RP_ERR_INVALID


def _objective(out):
    vel1, d0, d1 = out[:3]
    return ((d0 + d1) ** 2).sum() + torch.sin(vel1).sum()


def _expected_hvp(vel1, d0, d1, J, H, v):
    """(J^T f'' J + S_a f'_a H_a) v per problem for _objective: f' = (cos vel1, 2 (t0 + t1), 2 (t0 + t1))."""
    n = len(vel1)
    g = np.stack([np.cos(vel1), 2 * (d0 + d1), 2 * (d0 + d1)], axis=1)
    F = np.zeros((n, 3, 3))
    F[:, 0, 0] = -np.sin(vel1)
    F[:, 1:, 1:] = 2
    Hess = np.einsum("nab,nbc,ncd->nad", np.swapaxes(J, 1, 2), F, J) + np.einsum("na,nabc->nbc", g, H)
    return np.einsum("nbc,nc->nb", Hess, v), Hess


def test_double_backward_matches_min_time_hessian():
    n = 4096
    p = rp.problems.generate(131, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    pos = [_t(x).requires_grad_() for x in p]
    v = np.random.default_rng(22).standard_normal((n, 3))
    out = rp.min_time_solve(*pos)
    g = torch.autograd.grad(_objective(out), pos, create_graph=True)
    s = sum((gk * _t(v[:, k])).sum() for k, gk in enumerate(g))
    got = np.stack([x.detach().cpu().numpy() for x in torch.autograd.grad(s, pos)], axis=1)
    vel1, d0, d1, _, _, jac, hess = rp.min_time_hessian(*[x.detach() for x in pos])
    ref, _ = _expected_hvp(vel1.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy(), v)
    err = _rel(got, ref)
    print("double backward vs min_time_hessian: median %.2e, worst %.2e" % (np.median(err), err.max()))
    assert np.all(np.isfinite(got)) and err.max() <= 1e-12
    # only one position differentiated the second time: the other inputs' upstream gradients are None
    g1 = torch.autograd.grad(_objective(rp.min_time_solve(*pos)), pos[1], create_graph=True)[0]
    got1 = torch.autograd.grad((g1 * _t(v[:, 1])).sum(), pos[1])[0].cpu().numpy()
    e1 = np.stack([np.zeros(n), v[:, 1], np.zeros(n)], axis=1)
    ref1, _ = _expected_hvp(vel1.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy(), e1)
    assert np.all(np.abs(got1 - ref1[:, 1]) <= 1e-12 * np.abs(ref).max(axis=1))

    # torch.autograd.functional.hessian on 16 problems: the block-diagonal matrix of the per-problem Hessians
    m = 16
    q = [x.detach()[:m].clone() for x in pos]
    full = torch.autograd.functional.hessian(lambda a, b_, c: _objective(rp.min_time_solve(a, b_, c)), tuple(q))
    vel1, d0, d1, _, _, jac, hess = rp.min_time_hessian(*q)
    _, Hm = _expected_hvp(vel1.cpu().numpy(), d0.cpu().numpy(), d1.cpu().numpy(), jac.cpu().numpy(), hess.cpu().numpy(),
                          np.zeros((m, 3)))
    ref = np.zeros((3, 3, m, m))
    for b_ in range(3):
        for c in range(3):
            ref[b_, c] = np.diag(Hm[:, b_, c])
    got = np.stack([np.stack([full[b_][c].cpu().numpy() for c in range(3)]) for b_ in range(3)])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("functional.hessian vs min_time_hessian: %.2e" % err)
    assert err <= 1e-12


def test_first_order_gradients_unchanged_bit_for_bit():
    n = 4096
    p = rp.problems.generate(137, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    g = np.random.default_rng(23).standard_normal((n, 3))
    with jc._solved_batch(p) as b:
        ref = jc._device_vjp(b, g)
    for create_graph in (False, True):
        pos = [_t(x).requires_grad_() for x in p]
        out = rp.min_time_solve(*pos)
        grads = torch.autograd.grad(out[:3], pos, grad_outputs=[_t(g[:, k]) for k in range(3)], create_graph=create_graph)
        assert all(x.requires_grad == create_graph for x in grads)
        got = np.stack([x.detach().cpu().numpy() for x in grads], axis=1)
        assert np.array_equal(_bits(got), _bits(ref)), create_graph


def test_min_time_hessian_outputs_and_streams():
    n = 8192
    p, _ = jc._mixed(139, n)
    pos = [_t(x) for x in p]
    res = rp.min_time_hessian(*pos)
    assert len(res) == 7
    v, d0, d1, it, st, jac, hess = res
    assert jac.shape == (n, 3, 3) and hess.shape == (n, 3, 3, 3)
    assert jac.dtype == hess.dtype == torch.float64 and it.dtype == st.dtype == torch.int32
    assert not any(t.requires_grad for t in res)
    out = rp.min_time_solve(*[x.clone().requires_grad_() for x in pos])
    for a, b_ in zip((v, d0, d1, it, st), out):
        assert torch.equal(a, b_.detach())
    with jc._solved_batch(p) as b:
        Jd, Hd = _device_hessian(b)
    assert np.array_equal(_bits(hess.cpu().numpy()), _bits(Hd)) and np.array_equal(_bits(jac.cpu().numpy()), _bits(Jd))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res2 = rp.min_time_hessian(*pos)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b_ in zip(res2, res):
        assert np.array_equal(_bits(a.cpu().numpy().astype(np.float64)), _bits(b_.cpu().numpy().astype(np.float64)))


def test_pool_bound_and_double_backward_lease():
    n = 1024
    p = rp.problems.generate(149, 0, n, rp.problems.DIST_MONOTONE)
    pos = [_t(x) for x in p]
    autograd.clear_pool()
    for _ in range(200):
        rp.min_time_hessian(*pos)
    for _ in range(100):
        req = [x.clone().requires_grad_() for x in pos]
        g = torch.autograd.grad(_objective(rp.min_time_solve(*req)), req, create_graph=True)
        torch.autograd.grad(sum(x.sum() for x in g), req)
        del g, req
    gc.collect()
    torch.cuda.synchronize()
    sizes = {k: len(v) for k, v in autograd._pool._free.items()}
    print("pooled batches per key:", sizes)
    assert len(sizes) == 1 and all(v == 1 for v in sizes.values())
    key = next(iter(sizes))
    # a live double-backward graph holds its batch; it comes back once the graph is freed
    req = [x.clone().requires_grad_() for x in pos]
    out = rp.min_time_solve(*req)
    g = torch.autograd.grad(_objective(out), req, create_graph=True)
    del out
    gc.collect()
    assert len(autograd._pool._free.get(key, [])) == 0
    torch.autograd.grad(sum(x.sum() for x in g), req, retain_graph=True)
    assert len(autograd._pool._free.get(key, [])) == 0
    del g
    gc.collect()
    torch.cuda.synchronize()
    assert len(autograd._pool._free.get(key, [])) == 1


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
