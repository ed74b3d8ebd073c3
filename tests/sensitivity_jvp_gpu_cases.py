"""The cases of tests/test_gpu_sensitivity_jvp.py, each run in a fresh process (`python tests/sensitivity_jvp_gpu_cases.py <case>`):
torch must initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py).  Not collected by pytest (no
test_ prefix on the file)."""
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import rocket_path_amd as rp  # noqa: E402
import sensitivity_jvp_ref as jr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import autograd  # noqa: E402

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_jvp(b, td):
    """x_dot (n, 3) of Batch b for position tangents td (n, 3) host array."""
    ts = [_t(td[:, k]) for k in range(3)]
    outs = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    b.solution_jvp(*[x.data_ptr() for x in ts], *[x.data_ptr() for x in outs])
    b.sync()
    return np.stack([x.cpu().numpy() for x in outs], axis=1)


def _device_vjp(b, g):
    gs = [_t(g[:, k]) for k in range(3)]
    bars = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    b.solution_vjp(*[x.data_ptr() for x in gs], *[x.data_ptr() for x in bars])
    b.sync()
    return np.stack([x.cpu().numpy() for x in bars], axis=1)


def _device_jacobian(b):
    jac = torch.empty((b.n, 3, 3), dtype=torch.float64, device=DEV)
    b.solution_jacobian(jac.data_ptr())
    b.sync()
    return jac.cpu().numpy()


def _solved_batch(p, gap_tol=1e-8, max_iter=200):
    b = rp.Batch(len(p[0]), rp.VARIANT_F3, rp.DTYPE_F64, device=0)
    b.set_problems(*p)
    b.solve(gap_tol, max_iter, 0)
    return b


def _mixed(seed, n):
    """n problems: a third each of the monotone, reference-like and non-monotone distributions."""
    sizes = [n - 2 * (n // 3), n // 3, n // 3]
    parts = [rp.problems.generate(seed, 0, k, d) for k, d in
             zip(sizes, (rp.problems.DIST_MONOTONE, rp.problems.DIST_REFERENCE_LIKE, rp.problems.DIST_NON_MONOTONE))]
    return [np.concatenate(x) for x in zip(*parts)], np.repeat([0, 1, 2], sizes)


def _rel(a, b, axis=1):
    return np.linalg.norm(a - b, axis=axis) / np.linalg.norm(b, axis=axis)


def test_device_jvp_matches_longdouble_restatement():
    oracle = Oracle()
    n = 65536
    p, dist = _mixed(61, n)
    td = np.random.default_rng(8).standard_normal((n, 3))
    with _solved_batch(p) as b:
        states = b.get_state()
        dev = _device_jvp(b, td)
    ref = jr.full_jvp(oracle, states, td).astype(np.float64)
    assert np.all(np.isfinite(dev))
    err = _rel(dev, ref)
    for d in range(3):
        e = err[dist == d]
        print("dist %d, %d problems: device JVP vs longdouble median %.2e, 99.9 %% %.2e, worst %.2e"
              % (d, e.size, np.median(e), np.percentile(e, 99.9), e.max()))
    assert np.percentile(err, 99.9) <= 1e-11 and err.max() <= 1e-9


def test_duality_with_the_vjp_at_full_size():
    n = 1 << 20
    p = rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)      # bench.py's batch
    rng = np.random.default_rng(9)
    td, g = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    with _solved_batch(p) as b:
        xdot = _device_jvp(b, td)
        tbar = _device_vjp(b, g)
    err = np.abs(np.sum(g * xdot, axis=1) - np.sum(tbar * td, axis=1)) / (np.linalg.norm(g, axis=1) * np.linalg.norm(xdot, axis=1))
    print("1 Mi problems: <g, JVP(t)> vs <VJP(g), t>: median %.2e, 99.9 %% %.2e, worst %.2e"
          % (np.median(err), np.percentile(err, 99.9), err.max()))
    assert np.all(np.isfinite(err)) and err.max() <= 1e-11


def test_jacobian_consistency():
    n = 65536
    p, _ = _mixed(67, n)
    td = np.random.default_rng(10).standard_normal((n, 3))
    with _solved_batch(p) as b:
        J = _device_jacobian(b)
        xdot = _device_jvp(b, td)
        rows = np.stack([_device_vjp(b, np.tile(np.eye(3)[k], (n, 1))) for k in range(3)], axis=1)
    assert np.all(np.isfinite(J))
    scale = np.linalg.norm(J, axis=(1, 2))
    e_jvp = np.linalg.norm(np.einsum("nab,nb->na", J, td) - xdot, axis=1) / (scale * np.linalg.norm(td, axis=1))
    e_vjp = np.linalg.norm(J - rows, axis=(1, 2)) / scale
    e_tr = np.max(np.abs(J.sum(axis=2)), axis=1) / np.max(np.abs(J), axis=(1, 2))
    print("Jacobian vs JVP worst %.2e, vs VJP rows worst %.2e, row sums worst %.2e" % (e_jvp.max(), e_vjp.max(), e_tr.max()))
    assert e_jvp.max() <= 1e-12 and e_vjp.max() <= 1e-11 and e_tr.max() <= 1e-12


def _of_state(states, td):
    with rp.Batch(len(states), rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.set_state(states)
        return _device_jvp(b, td), _device_jacobian(b)


def test_problem_order_on_pipeline_batch_and_after_nudge_equals_set_state():
    n = 8192
    p = rp.problems.generate(71, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    td = np.random.default_rng(11).standard_normal((n, 3))
    with rp.Pipeline(n, depth=2, n_streams=2) as pl:
        pos = [_t(x) for x in p]
        torch.cuda.synchronize()
        job = pl.submit(*[x.data_ptr() for x in pos])
        pl.wait(job)
        b = pl.batch(job)
        got = _device_jvp(b, td), _device_jacobian(b)
        states = b.get_state()
    ref = _of_state(states, td)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    for a, r in zip(got, ref):
        assert np.array_equal(_bits(a), _bits(r))
    with _solved_batch(p) as b:
        b.nudge(0, 0.25)      # vel1 += 0.25: a state off the central path, still inside
        got = _device_jvp(b, td), _device_jacobian(b)
        states = b.get_state()
    for a, r in zip(got, _of_state(states, td)):
        assert np.array_equal(_bits(a), _bits(r))
    # a NULL tangent counts as zeros; equal tangents on all three positions give exactly 0
    with _solved_batch(p) as b:
        t0 = td.copy()
        t0[:, 1] = 0
        outs = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(3)]
        ts = [_t(td[:, 0]), None, _t(td[:, 2])]
        b.solution_jvp(*[x.data_ptr() if x is not None else 0 for x in ts], *[x.data_ptr() for x in outs])
        b.sync()
        assert np.array_equal(_bits(np.stack([x.cpu().numpy() for x in outs], axis=1)), _bits(_device_jvp(b, t0)))
        same = np.repeat(td[:, :1], 3, axis=1)
        assert np.all(_device_jvp(b, same) == 0)


def test_nan_rows_and_unsupported_modes():
    n = 4096
    p = rp.problems.generate(73, 0, n, rp.problems.DIST_MONOTONE)
    with _solved_batch(p) as b:
        states = b.get_state()
    bad_inf = np.arange(0, n, 7)
    bad_nan = np.arange(3, n, 11)
    states[bad_inf, 1] *= 0.1      # duration0 / 10: accelerations x 100, outside |a| <= L
    states[bad_nan, 5] = np.nan
    bad = np.zeros(n, dtype=bool)
    bad[bad_inf] = bad[bad_nan] = True
    assert np.array_equal(jr.condensed(states)["ok"], ~bad)
    td = np.random.default_rng(12).standard_normal((n, 3))
    xdot, J = _of_state(states, td)
    assert np.all(np.isnan(xdot[bad])) and np.all(np.isfinite(xdot[~bad]))
    assert np.all(np.isnan(J[bad])) and np.all(np.isfinite(J[~bad]))
    for variant, dtype in ((rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F3, rp.DTYPE_F32), (rp.VARIANT_F3, rp.DTYPE_F32_STATE)):
        with rp.Batch(64, variant, dtype, device=0) as b:
            b.init_default()
            for call in (lambda: b.solution_jvp(0, 0, 0, 0, 0, 0), lambda: b.solution_jacobian(0)):
                with pytest.raises(rp.RpError) as e:
                    call()
                assert e.value.status == rp.capi.RP_ERR_UNSUPPORTED, (variant, dtype)
    with rp.Batch(64, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
        b.init_default()
        for call in (lambda: b.solution_jvp(0, 0, 0, 0, 0, 0), lambda: b.solution_jacobian(0)):
            with pytest.raises(rp.RpError) as e:
                call()
            assert e.value.status == rp.capi.RP_ERR_INVALID


def test_forward_ad_equals_batch_path_bit_for_bit():
    n = 4096
    p = rp.problems.generate(79, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    td = np.random.default_rng(13).standard_normal((n, 3))
    pos, tan = [_t(x) for x in p], [_t(td[:, k]) for k in range(3)]
    with _solved_batch(p) as b:
        ref = _device_jvp(b, td)
        only1 = td.copy()
        only1[:, 0] = only1[:, 2] = 0
        ref1 = _device_jvp(b, only1)
    with fwAD.dual_level():
        out = rp.min_time_solve(*[fwAD.make_dual(x, t) for x, t in zip(pos, tan)])
        got = np.stack([fwAD.unpack_dual(o).tangent.cpu().numpy() for o in out[:3]], axis=1)
        assert fwAD.unpack_dual(out[3]).tangent is None
        out = rp.min_time_solve(pos[0], fwAD.make_dual(pos[1], tan[1]), pos[2])
        got1 = np.stack([fwAD.unpack_dual(o).tangent.cpu().numpy() for o in out[:3]], axis=1)
    assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(got1), _bits(ref1))
    primals, tangents = torch.func.jvp(lambda a, b_, c: rp.min_time_solve(a, b_, c)[:3], tuple(pos), tuple(tan))
    got = np.stack([t.cpu().numpy() for t in tangents], axis=1)
    assert np.array_equal(_bits(got), _bits(ref))
    with _solved_batch(p) as b:
        st = b.get_state()
    for k in range(3):
        assert np.array_equal(_bits(primals[k].cpu().numpy()), _bits(st[:, k]))


def test_forward_ad_matches_finite_differences():
    n = 4096
    p = rp.problems.generate(83, 0, n, rp.problems.DIST_MONOTONE)
    td = np.random.default_rng(14).standard_normal((n, 3))
    with fwAD.dual_level():
        out = rp.min_time_solve(*[fwAD.make_dual(_t(x), _t(td[:, k])) for k, x in enumerate(p)], gap_tol=1e-13)
        xdot = np.stack([fwAD.unpack_dual(o).tangent.cpu().numpy() for o in out[:3]], axis=1)
        st = out[4].cpu().numpy()
    outside = (st & (rp.ST_NONFINITE | rp.ST_INFEASIBLE)) != 0
    assert np.all(np.isfinite(xdot[~outside])) and np.all(np.isnan(xdot[outside]))

    def solve(q):
        with _solved_batch(q, gap_tol=1e-13) as b:
            return b.get_state()
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1])) / np.max(np.abs(td), axis=1)
    base = solve(p)
    lo = solve([x - h * td[:, k] for k, x in enumerate(p)])
    hi = solve([x + h * td[:, k] for k, x in enumerate(p)])
    fd = (hi[:, :3] - lo[:, :3]) / (2 * h[:, None])
    act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
    ok = ~outside & np.all((act(base) == act(lo)) & (act(base) == act(hi)), axis=1)
    err = _rel(xdot[ok], fd[ok])
    print("forward AD vs finite differences: %d of %d active-set-stable (%d outside the feasible set), median %.2e, worst %.2e"
          % (ok.sum(), n, outside.sum(), np.median(err), err.max()))
    assert ok.mean() > 0.9 and err.max() <= 1e-5


def test_reverse_mode_unchanged_bit_for_bit():
    n = 4096
    p = rp.problems.generate(89, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    g = np.random.default_rng(15).standard_normal((n, 3))
    pos = [_t(x).requires_grad_() for x in p]
    out = rp.min_time_solve(*pos)
    grads = torch.autograd.grad(out[:3], pos, grad_outputs=[_t(g[:, k]) for k in range(3)])
    got = np.stack([x.cpu().numpy() for x in grads], axis=1)
    with _solved_batch(p) as b:
        ref = _device_vjp(b, g)
    assert np.array_equal(_bits(got), _bits(ref))


def test_min_time_jacobian_matches_reverse_passes_and_streams():
    n = 8192
    p, dist = _mixed(97, n)
    pos = [_t(x) for x in p]
    v, d0, d1, it, st, jac = rp.min_time_jacobian(*pos)
    assert jac.shape == (n, 3, 3) and jac.dtype == torch.float64 and not jac.requires_grad
    J = jac.cpu().numpy()
    req = [x.clone().requires_grad_() for x in pos]
    out = rp.min_time_solve(*req)
    rows = []
    for k in range(3):
        gk = torch.autograd.grad(out[k], req, grad_outputs=torch.ones(n, dtype=torch.float64, device=DEV), retain_graph=k < 2)
        rows.append(np.stack([x.cpu().numpy() for x in gk], axis=1))
    rows = np.stack(rows, axis=1)
    for a, b_ in ((v, out[0]), (d0, out[1]), (d1, out[2]), (it, out[3]), (st, out[4])):
        assert torch.equal(a, b_.detach())
    err = np.linalg.norm(J - rows, axis=(1, 2)) / np.linalg.norm(J, axis=(1, 2))
    regular, degenerate = err[dist < 2], err[dist == 2]
    print("min_time_jacobian vs three reverse passes: worst %.2e (monotone, reference-like), %.2e (non-monotone)"
          % (regular.max(), degenerate.max()))
    # the degenerate non-monotone optima carry the condensed form's larger error (2e-13 on the CPU restatement)
    assert np.all(np.isfinite(J)) and regular.max() <= 1e-13 and degenerate.max() <= 1e-12
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = rp.min_time_jacobian(*pos)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(res[5].cpu().numpy()), _bits(J))
    for a, b_ in zip(res[:5], (v, d0, d1, it, st)):
        assert torch.equal(a, b_)


def test_pool_holds_one_batch_per_key():
    n = 1024
    p = rp.problems.generate(101, 0, n, rp.problems.DIST_MONOTONE)
    pos = [_t(x) for x in p]
    tan = [_t(np.random.default_rng(16).standard_normal(n)) for _ in range(3)]
    autograd.clear_pool()
    with torch.no_grad():
        for _ in range(1000):
            rp.min_time_solve(*[x.clone().requires_grad_() for x in pos])
    with fwAD.dual_level():
        for _ in range(1000):
            out = rp.min_time_solve(*[fwAD.make_dual(x, t) for x, t in zip(pos, tan)])
            del out
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(50):
            rp.min_time_jacobian(*pos)
    torch.cuda.synchronize()
    sizes = {k: len(v) for k, v in autograd._pool._free.items()}
    print("pooled batches per key:", sizes)
    assert len(sizes) == 2 and all(v == 1 for v in sizes.values())


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
