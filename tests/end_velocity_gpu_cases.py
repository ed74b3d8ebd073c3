"""The cases of tests/test_gpu_end_velocity.py, each run in a fresh process (`python tests/end_velocity_gpu_cases.py <case>`): torch
must initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py).  Not collected by pytest (no test_
prefix on the file)."""
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import end_velocity_ref as er  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import autograd  # noqa: E402
from parity_util import certify_iteration_counts, keep_mask  # noqa: E402

DEV = "cuda:0"
N = 65536


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _inputs(orc, kappa, n=N, seed=41):
    """n problems of all three generators (thirds) with end velocities kappa U(-1, 1) sqrt(L |dX|)."""
    parts = [er.velocities(orc, d, kappa, n // 3 + 1, seed + d) for d in range(3)]
    return [np.concatenate([p[k] for p in parts])[:n] for k in range(5)]


def _set_vel(b, args, nulls=False):
    ts = [_t(a) for a in args]
    b.set_problems_vel_device(*[t.data_ptr() for t in ts[:3]], *((0, 0) if nulls else [t.data_ptr() for t in ts[3:]]))
    b.sync()


def _vjp_vel(b, g):
    gs = [_t(g[:, k]) for k in range(3)]
    outs = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(5)]
    b.solution_vjp_vel(*[x.data_ptr() for x in gs], *[x.data_ptr() for x in outs])
    b.sync()
    return np.stack([x.cpu().numpy() for x in outs], axis=1)


def _jvp_vel(b, td):
    ts = [_t(td[:, k]) for k in range(5)]
    outs = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    b.solution_jvp_vel(*[x.data_ptr() for x in ts], *[x.data_ptr() for x in outs])
    b.sync()
    return np.stack([x.cpu().numpy() for x in outs], axis=1)


def _jac_vel(b):
    J = torch.empty((b.n, 3, 5), dtype=torch.float64, device=DEV)
    b.solution_jacobian_vel(J.data_ptr())
    b.sync()
    return J.cpu().numpy()


def _old(b, g, td):
    """the existing kernels: VJP (n, 3), JVP (n, 3) along the position tangents td[:, :3], Jacobian (n, 3, 3)"""
    gs = [_t(g[:, k]) for k in range(3)]
    ts = [_t(td[:, k]) for k in range(3)]
    vo = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    jo = [torch.empty(b.n, dtype=torch.float64, device=DEV) for _ in range(3)]
    J = torch.empty((b.n, 3, 3), dtype=torch.float64, device=DEV)
    b.solution_vjp(*[x.data_ptr() for x in gs], *[x.data_ptr() for x in vo])
    b.solution_jvp(*[x.data_ptr() for x in ts], *[x.data_ptr() for x in jo])
    b.solution_jacobian(J.data_ptr())
    b.sync()
    return np.stack([x.cpu().numpy() for x in vo], axis=1), np.stack([x.cpu().numpy() for x in jo], axis=1), J.cpu().numpy()


def test_zero_and_null_velocities_equal_set_problems_device():
    orc = Oracle()
    args = _inputs(orc, 0.0)
    with rp.Batch(N) as ref:
        ts = [_t(a) for a in args[:3]]
        ref.set_problems_device(*[t.data_ptr() for t in ts])
        ref.solve(1e-8, 200, 0)
        it_r, st_r = ref.get_iters(), ref.get_state()
    for nulls in (False, True):
        with rp.Batch(N) as b:
            _set_vel(b, args, nulls)
            b.solve(1e-8, 200, 0)
            it, st = b.get_iters(), b.get_state()
        assert np.array_equal(it[0], it_r[0]) and np.array_equal(it[1], it_r[1]), nulls
        diff = _bits(st) != _bits(st_r)
        print("nulls %s: %d of %d state words differ in their bits, in fields %s; values equal: %s"
              % (nulls, int(diff.sum()), diff.size, sorted(set(np.nonzero(diff)[1].tolist())), np.array_equal(st, st_r, equal_nan=True)))
        assert np.array_equal(st, st_r, equal_nan=True), nulls


def test_start_solve_and_restart_with_velocities():
    orc = Oracle()
    for kappa in (0.1, 0.3):
        args = _inputs(orc, kappa)
        start = er.start_state(*args)
        with rp.Batch(N) as b:
            _set_vel(b, args)
            assert np.array_equal(_bits(b.get_state()), _bits(start)), "start"
            b.solve(1e-8, 200, 0)
            it, status = b.get_iters()
            st = b.get_state()
            b.restart()
            assert np.array_equal(_bits(b.get_state()), _bits(start)), "restart"
            assert np.all(b.get_iters()[0] == 0)
        ref = start.copy()
        it_ref, _ = orc.batch_solve_gated(3, ref, 1e-8, 200)
        conv = (status & rp.capi.ST_CONVERGED) != 0
        hist = np.bincount(np.minimum(it, 200), minlength=201)
        print("kappa %g: converged %.4f, mean steps %.2f, iteration histogram %s"
              % (kappa, conv.mean(), it.mean(), {int(k): int(v) for k, v in enumerate(hist) if v}))
        # kappa 0.1: every problem; 0.3: the problems the oracle converges (the others drift towards t = 0 or infinity, where two
        # correct evaluations of the same step may round a line-search decision differently)
        sel = np.ones(N, bool) if kappa == 0.1 else (it_ref < 200) & np.all(np.isfinite(ref), axis=1)
        if kappa != 0.1:      # near the t = 0 wall a line-search decision can round either way: measured 11 of 65,041 problems
            other = sel & (it != it_ref)
            print("kappa %g: %d of %d oracle-converged problems take another step count" % (kappa, int(other.sum()), int(sel.sum())))
            assert other.sum() <= 5e-4 * sel.sum()
            sel &= ~other
        ties = certify_iteration_counts(orc, 3, start[sel], it[sel], it_ref[sel], 1e-8)
        ok = keep_mask(int(sel.sum()), ties)
        a, r = st[sel][ok], ref[sel][ok]
        e = np.max(np.abs(a[:, :3] - r[:, :3]) / np.maximum(np.abs(r[:, :3]), 1.0), axis=1)
        print("kappa %g: %d problems compared, %d gate ties, state error median %.2e, 99.9 %% %.2e, worst %.2e, %d above 1e-10"
              % (kappa, int(sel.sum()), len(ties), np.median(e), np.quantile(e, 0.999), e.max(), int((e > 1e-10).sum())))
        # identical step counts; the states agree to 1e-10 but for a few problems per thousand whose last steps are ill-conditioned
        # (the device condenses the Newton system, the oracle runs the reference's QR): there within O(gap)
        assert np.quantile(e, 0.99) < 1e-10 and e.max() < 1e-6


def test_f4_and_f32_state_start_and_fixed_steps():
    orc = Oracle()
    n = 4096
    args = _inputs(orc, 0.1, n)
    for variant, dtype, storage, k, tol in ((rp.VARIANT_F4, rp.DTYPE_F64, np.float64, 5, 1e-9),
                                            (rp.VARIANT_F3, rp.DTYPE_F32_STATE, np.float32, 1, 1e-6)):
        start = er.start_state(*args, variant=variant, storage=storage)
        with rp.Batch(n, variant, dtype) as b:
            _set_vel(b, args)
            assert np.array_equal(_bits(b.get_state()), _bits(start)), (variant, dtype)
            b.step(k)
            st = b.get_state()
        ref = orc.batch_steps(variant, start.copy(), k)
        fin = np.all(np.isfinite(ref), axis=1)
        err = np.max(np.abs(st[fin, :3] - ref[fin, :3]) / np.maximum(np.abs(ref[fin, :3]), 1.0))
        print("variant %d dtype %d: %d steps, max error %.2e" % (variant, dtype, k, err))
        assert err < tol


def test_every_start_form_follows_the_one_rule():
    """k_start_from_records and k_restart_feasible in every number mode: the written start, a restart (with end velocities: only F3 /
    float64 restarts anywhere else) and the zero-velocity form against set_problems_device.  Two full blocks and a ragged one."""
    orc = Oracle()
    n = 2 * 256 + 17
    args = _inputs(orc, 0.1, n)
    args[3][[0, 5, 255, 256, n - 1]] = -0.0      # stored as +0
    args[4][[1, 5, 511, 512, n - 1]] = -0.0
    zeros = np.zeros(n)
    for variant, dtype, storage in ((rp.VARIANT_F3, rp.DTYPE_F64, np.float64), (rp.VARIANT_F3, rp.DTYPE_F32_STATE, np.float32),
                                    (rp.VARIANT_F4, rp.DTYPE_F64, np.float64), (rp.VARIANT_F4, rp.DTYPE_F32, np.float32)):
        mode = (variant, dtype)
        with rp.Batch(n, variant, dtype) as b:
            # both velocities given, then vel0 NULL and vel2 given: the written start, and the same start again after a restart
            for given in (args, args[:3] + [zeros, args[4]]):
                start = er.start_state(*given, variant=variant, storage=storage)
                ts = [_t(a) for a in given]
                b.set_problems_vel_device(*[t.data_ptr() for t in ts[:3]], ts[3].data_ptr() if given is args else 0, ts[4].data_ptr())
                b.sync()
                assert np.array_equal(_bits(b.get_state()), _bits(start)), ("start", mode, given is args)
                b.step(2)
                assert not np.array_equal(_bits(b.get_state()), _bits(start)), ("stepped", mode)
                b.restart()
                assert np.array_equal(_bits(b.get_state()), _bits(start)), ("restart", mode, given is args)
                assert np.all(b.get_iters()[0] == 0), ("restart", mode)
            # zero velocities: the bits set_problems_device leaves in a second batch
            _set_vel(b, args[:3] + [zeros, zeros])
            with rp.Batch(n, variant, dtype) as rest:
                ts = [_t(a) for a in args[:3]]
                rest.set_problems_device(*[t.data_ptr() for t in ts])
                rest.sync()
                assert np.array_equal(_bits(b.get_state()), _bits(rest.get_state())), ("zero velocities", mode)


def test_derivative_kernels_against_longdouble_and_existing_kernels():
    orc = Oracle()
    for kappa in (0.0, 0.1, 0.3):
        args = _inputs(orc, kappa)
        with rp.Batch(N) as b:
            _set_vel(b, args)
            b.solve(1e-13, 200, 0)
            st = b.get_state()
            b_status = b.get_iters()[1]
            rng = np.random.default_rng(9)
            g, td = rng.standard_normal((N, 3)), rng.standard_normal((N, 5))
            vjp, jvp, J = _vjp_vel(b, g), _jvp_vel(b, td), _jac_vel(b)
            td0 = td.copy()
            td0[:, 3:] = 0
            jvp0 = _jvp_vel(b, td0)
            vo, jo, Jo = _old(b, g, td)
        fin = np.all(np.isfinite(J.reshape(N, -1)), axis=1)
        assert np.array_equal(fin, np.all(np.isfinite(vjp), axis=1)) and np.array_equal(fin, np.all(np.isfinite(jvp), axis=1))
        # compared: the problems that converged to positive durations (the others drift)
        ok = fin & (b_status & rp.capi.ST_CONVERGED != 0) & (st[:, 1] > 0) & (st[:, 2] > 0)
        cons = (er.rel(np.einsum("nab,nb->na", J[ok], td[ok]), jvp[ok]), er.rel(np.einsum("na,nab->nb", g[ok], J[ok]), vjp[ok]))
        print("kappa %g: %d finite, %d compared; Jacobian vs JVP worst %.2e, vs VJP worst %.2e"
              % (kappa, int(fin.sum()), int(ok.sum()), cons[0].max(), cons[1].max()))
        # position parts: the existing kernels
        assert np.max(er.rel(J[ok][:, :, :3], Jo[ok])) <= 1e-14
        assert np.max(er.rel(vjp[ok][:, :3], vo[ok])) <= 1e-14
        assert np.max(er.rel(jvp0[ok], jo[ok])) <= 1e-14
        # Jacobian columns against the JVP, rows against the VJP
        assert cons[0].max() < 1e-12 and cons[1].max() < 1e-12
        # against the longdouble system on a sample, away from the degenerate four-active states (tests/test_end_velocity_cpu.py)
        idx = np.flatnonzero(ok & ((st[:, 3:11] > 1e-6).sum(axis=1) < 4))[:: 16]
        Jf = er.full_jacobian5(st[idx]).astype(np.float64)
        e = er.rel(J[idx], Jf)
        print("kappa %g: %d NaN rows; vs longdouble on %d rows: worst %.2e, median %.2e" % (kappa, (~fin).sum(), len(idx), e.max(), np.median(e)))
        assert e.max() < 1e-10


def test_autograd_and_forward_ad_against_differences():
    orc = Oracle()
    n = 4096
    p0, p1, p2, v0, v2 = _inputs(orc, 0.1, n)
    pos = [_t(a) for a in (p0, p1, p2)]
    vel = [_t(a).requires_grad_() for a in (v0, v2)]
    out = rp.min_time_solve(*pos, vel0=vel[0], vel2=vel[1], gap_tol=1e-13)
    w = torch.tensor([0.1, 1.0, 1.0], dtype=torch.float64, device=DEV)
    loss = (torch.stack(out[:3], 1) * w).sum()
    gv0, gv2 = torch.autograd.grad(loss, vel)
    ok = ((out[4] & rp.capi.ST_CONVERGED) != 0) & torch.isfinite(gv0) & torch.isfinite(gv2)
    # central differences of the device solve in each velocity
    h = 1e-4
    fd = []
    for k in range(2):
        xs = []
        for sgn in (1, -1):
            vv = [t.detach().clone() for t in vel]
            vv[k] += sgn * h
            xs.append(torch.stack(rp.min_time_solve(*pos, vel0=vv[0], vel2=vv[1], gap_tol=1e-13)[:3], 1))
        fd.append(((xs[0] - xs[1]) / (2 * h) * w).sum(1))
    rel0 = ((gv0 - fd[0]).abs() / fd[0].abs().clamp(min=1e-3))[ok]
    rel2 = ((gv2 - fd[1]).abs() / fd[1].abs().clamp(min=1e-3))[ok]
    print("reverse mode vs differences on %d problems: median %.2e / %.2e, 95 %% %.2e / %.2e"
          % (int(ok.sum()), rel0.median(), rel2.median(), rel0.quantile(0.95), rel2.quantile(0.95)))
    assert ok.float().mean() > 0.95
    assert rel0.median() < 1e-5 and rel2.median() < 1e-5 and rel0.quantile(0.95) < 1e-3 and rel2.quantile(0.95) < 1e-3
    # forward mode: forward_ad and torch.func.jvp against the Jacobian
    jac = rp.min_time_jacobian(*pos, vel0=vel[0].detach(), vel2=vel[1].detach(), gap_tol=1e-13)[5]
    assert jac.shape == (n, 3, 5)
    good = torch.isfinite(jac.reshape(n, -1)).all(1)
    tv = torch.randn(n, dtype=torch.float64, device=DEV)
    with fwAD.dual_level():
        dv = fwAD.make_dual(vel[0].detach(), tv)
        o = rp.min_time_solve(*pos, vel0=dv, vel2=vel[1].detach(), gap_tol=1e-13)
        tang = torch.stack([fwAD.unpack_dual(t).tangent for t in o[:3]], 1)
    ref = jac[:, :, 3] * tv[:, None]
    assert torch.allclose(tang[good], ref[good], rtol=1e-12, atol=1e-12 * ref[good].abs().max().item())

    def f(a, b):
        return rp.min_time_solve(*pos, vel0=a, vel2=b, gap_tol=1e-13)[1]
    _, t2 = torch.func.jvp(f, (vel[0].detach(), vel[1].detach()), (torch.zeros_like(tv), tv))
    ref2 = jac[:, 1, 4] * tv
    assert torch.allclose(t2[good], ref2[good], rtol=1e-12, atol=1e-12 * ref2[good].abs().max().item())
    # min_time_hessian: the (n, 3, 5) Jacobian and the positions-only Hessian at that state
    hout = rp.min_time_hessian(*pos, vel0=vel[0].detach(), vel2=vel[1].detach(), gap_tol=1e-13)
    assert hout[5].shape == (n, 3, 5) and hout[6].shape == (n, 3, 3, 3)
    assert torch.equal(hout[5][good], jac[good])
    # first order only: a double backward raises torch's once_differentiable error
    out = rp.min_time_solve(*pos, vel0=vel[0], vel2=vel[1])
    g0, = torch.autograd.grad((out[1] ** 2).sum(), vel[0], create_graph=True)
    try:
        g0.sum().backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("double backward did not raise")
    torch.cuda.synchronize()


def test_pool_reuse_after_velocities_is_bit_identical():
    orc = Oracle()
    n = 4096
    p0, p1, p2, v0, v2 = _inputs(orc, 0.3, n)
    pos = [_t(a) for a in (p0, p1, p2)]
    autograd.clear_pool()
    fresh = [t.clone() for t in rp.min_time_solve(*pos)]
    torch.cuda.synchronize()
    for _ in range(2):
        rp.min_time_solve(*pos, vel0=_t(v0), vel2=_t(v2))
        again = rp.min_time_solve(*pos)
        torch.cuda.synchronize()
        for a, b in zip(fresh, again):
            assert torch.equal(a, b)
    sizes = {k: len(v) for k, v in autograd._pool._free.items()}
    assert len(sizes) == 1 and all(v == 1 for v in sizes.values()), sizes


def test_batch_edges_and_padding():
    orc = Oracle()
    big = 8192
    args = _inputs(orc, 0.1, big)
    with rp.Batch(big) as b:
        _set_vel(b, args)
        b.solve(1e-8, 200, 0)
        st_big = b.get_state()
        it_big = b.get_iters()[0]
        J_big = _jac_vel(b)
    for n in (1, 63, 64, 65, 4097):
        sub = [a[:n] for a in args]
        with rp.Batch(n) as b:
            _set_vel(b, sub)
            b.solve(1e-8, 200, 0)
            st = b.get_state()
            it = b.get_iters()[0]
            # padding: the element one past the end of every output stays untouched
            J = torch.full((n + 1, 3, 5), 7.0, dtype=torch.float64, device=DEV)
            b.solution_jacobian_vel(J.data_ptr())
            bars = [torch.full((n + 1,), 7.0, dtype=torch.float64, device=DEV) for _ in range(5)]
            b.solution_vjp_vel(0, 0, 0, *[x.data_ptr() for x in bars])
            dots = [torch.full((n + 1,), 7.0, dtype=torch.float64, device=DEV) for _ in range(3)]
            b.solution_jvp_vel(0, 0, 0, 0, 0, *[x.data_ptr() for x in dots])
            b.sync()
            J = J.cpu().numpy()
        # another batch, another internal order: the same per-problem arithmetic
        assert np.array_equal(it, it_big[:n]) and np.array_equal(_bits(st), _bits(st_big[:n])), n
        assert np.array_equal(_bits(J[:n]), _bits(J_big[:n])), n
        assert np.all(J[n] == 7.0) and all(float(x[n]) == 7.0 for x in bars + dots), n


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
