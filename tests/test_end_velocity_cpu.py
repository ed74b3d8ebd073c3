"""Problems with end velocities and the first derivatives in them, without a GPU: the new entries are declared,
bound and exported and reject a NULL handle; the torch layer's checks of the velocity tensors; the analytic velocity columns of dr/dtheta
against central differences of the longdouble residual; the kernels' condensed double-double arithmetic (tests/end_velocity_ref.py)
against the longdouble 11 x 11 system on the kappa in {0, 0.1, 0.3} families; translation, homogeneity and duality; the start rule's
feasibility."""
import ctypes

import numpy as np
import pytest

import end_velocity_ref as er
import sensitivity_hess_ref as hr
import sensitivity_jvp_ref as jr
import rocket_path_amd as rp
from rocket_path_amd import capi

NEW = ["rp_batch_set_problems_vel", "rp_batch_set_problems_vel_device", "rp_batch_solution_vjp_vel", "rp_batch_solution_jvp_vel",
       "rp_batch_solution_jacobian_vel"]
DISTS = [0, 1, 2]


def test_new_entries_are_declared_bound_and_reject_a_null_handle():
    assert capi.ABI_VERSION == 7
    lib = rp.load_library()
    assert lib.rp_abi_version() == 7
    hdr = open(capi.os.path.join(capi._HERE, "..", "include", "rp_batch.h")).read()
    for name in NEW:
        assert name in capi.SIGNATURES and "RP_API int %s(" % name in hdr
        fn = getattr(lib, name)
        assert fn(*([None] * len(capi.SIGNATURES[name][1]))) == capi.RP_ERR_INVALID


def test_torch_rejects_velocities_of_the_wrong_type_or_device():
    torch = pytest.importorskip("torch")
    from rocket_path_amd import autograd
    p = torch.zeros(4, dtype=torch.float64)
    for who in ("min_time_solve", "min_time_jacobian", "min_time_hessian"):
        with pytest.raises(TypeError):
            autograd._check_velocities(p, torch.zeros(4, dtype=torch.float64), None, who)      # not on a ROCm device
        with pytest.raises(TypeError):
            autograd._check_velocities(p, None, torch.zeros(4, dtype=torch.float32), who)
        with pytest.raises(TypeError):
            autograd._check_velocities(p, [0.0] * 4, None, who)
    assert autograd._check_velocities(p, None, None, "min_time_solve") is False
    with pytest.raises(TypeError):
        rp.min_time_solve(p, p, p, vel0=p)


@pytest.mark.parametrize("dist", DISTS)
def test_velocity_columns_match_central_differences_of_the_residual(oracle, dist):
    _, _, st, _ = er.family(oracle, dist, 0.3, 1e-8, n=128)
    st = st[np.all(np.isfinite(st), axis=1) & (st[:, 1] > 0) & (st[:, 2] > 0)]
    p = np.full(len(st), 1e-3)
    D = er.drdtheta5(st)
    for col, field in ((3, 12), (4, 15)):
        h = np.maximum(np.abs(st[:, field]), 1.0).astype(er.LD) * er.LD(1e-6)
        a, b = st.astype(er.LD), st.astype(er.LD)
        a[:, field] += h
        b[:, field] -= h
        fd = (hr.residual_ld(a, p) - hr.residual_ld(b, p)) / (2 * h[:, None])
        err = np.abs(fd - D[:, :, col]).max(axis=1) / np.maximum(np.abs(D[:, :, col]).max(axis=1), 1e-30)
        assert err.max() < 1e-7, err.max()


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("kappa", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
def test_condensed_arithmetic_matches_the_longdouble_system(oracle, dist, kappa, gap_tol):
    _, _, st, _ = er.family(oracle, dist, kappa, gap_tol, n=512)
    n = len(st)
    rng = np.random.default_rng(3)
    g, td = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    vjp, jvp, J = er.condensed_vjp5(st, g), er.condensed_jvp5(st, td), er.condensed_jacobian5(st)
    ok = np.all(np.isfinite(J.reshape(n, -1)), axis=1)
    assert np.array_equal(ok, np.all(np.isfinite(vjp), axis=1)) and np.array_equal(ok, np.all(np.isfinite(jvp), axis=1))
    assert ok.mean() > 0.9 if kappa < 0.3 else ok.mean() > 0.8
    Jf = er.full_jacobian5(st[ok]).astype(np.float64)
    # A state with all four accelerations at the limit (the non-monotone generator's rest-to-rest optimum: vel1 = 0, both segments
    # bang-bang) has four active constraints on three unknowns: there the velocity columns are set by the ratios of the four D_j,
    # i.e. by c_j ~ p / lam, which float64 a - L carries to eps L / |c| only (measured: <= 9e-7 at gap 1e-8, <= 7e-2 at 1e-13).  The
    # position columns are unaffected (<= 2e-14), and so is every other state.
    four = (st[ok][:, 3:11] > 1e-6).sum(axis=1) >= 4
    assert four.mean() < 0.05 or (dist == 2 and kappa == 0.0)
    pos = er.rel(J[ok][:, :, :3], Jf[:, :, :3])
    keep = ~four
    errs = (er.rel(J[ok], Jf)[keep], er.rel(vjp[ok], np.einsum("na,nab->nb", g[ok], Jf))[keep],
            er.rel(jvp[ok], np.einsum("nab,nb->na", Jf, td[ok]))[keep])
    worst = max(e.max() for e in errs)
    print("dist %d kappa %g gap %g: worst %.2e (Jacobian %.2e VJP %.2e JVP %.2e), position columns %.2e, %d NaN rows, %d with four "
          "active constraints" % (dist, kappa, gap_tol, worst, errs[0].max(), errs[1].max(), errs[2].max(), pos.max(), (~ok).sum(), four.sum()))
    assert worst < 1e-10 and pos.max() < 1e-10
    # the position columns are the existing kernels' arithmetic
    np.testing.assert_array_equal(J[ok][:, :, :3], jr.condensed_jacobian(st[ok]))


@pytest.mark.parametrize("dist", DISTS)
def test_translation_homogeneity_and_duality(oracle, dist):
    (p0, p1, p2, v0, v2), _, st, _ = er.family(oracle, dist, 0.1, 1e-13, n=512)
    n = len(st)
    J = er.condensed_jacobian5(st)
    ok = np.all(np.isfinite(J.reshape(n, -1)), axis=1)
    assert ok.mean() > 0.95
    J, s = J[ok], st[ok]
    assert np.abs(J[:, :, :3].sum(axis=2)).max() <= 1e-9 * np.abs(J[:, :, :3]).max()      # translation: S pos_bar = 0
    # homogeneity: x(lambda pos, sqrt(lambda) vel) = sqrt(lambda) x at the optimum
    theta = np.stack([s[:, 11], s[:, 13], s[:, 14], 0.5 * s[:, 12], 0.5 * s[:, 15]], axis=1)
    lhs = np.einsum("nab,nb->na", J, theta)
    x = s[:, :3]
    err = np.abs(lhs - x / 2).max(axis=1) / np.abs(x).max(axis=1)
    assert np.median(err) < 1e-6 and np.quantile(err, 0.99) < 1e-3, (np.median(err), np.quantile(err, 0.99))
    # duality of the VJP and JVP restatements
    rng = np.random.default_rng(5)
    g, td = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    a = np.einsum("na,na->n", g, er.condensed_jvp5(st, td))[ok]
    b = np.einsum("nb,nb->n", er.condensed_vjp5(st, g), td)[ok]
    assert (np.abs(a - b) / np.maximum(np.abs(a), 1.0)).max() < 1e-10


@pytest.mark.parametrize("kappa", [0.1, 1.0, 3.0])
def test_start_rule_is_strictly_feasible_and_rest_to_rest_at_zero(oracle, kappa):
    for dist in DISTS:
        p0, p1, p2, v0, v2 = er.velocities(oracle, dist, kappa, 2048, 7)
        st = er.start_state(p0, p1, p2, v0, v2)
        for i in range(len(st)):
            for c in range(8):
                assert oracle.constraint(3, c, st[i])[0] <= -0.02 * er.L_DEFAULT + 1e-9
        z = er.start_state(p0, p1, p2, 0 * v0, 0 * v2)
        np.testing.assert_array_equal(z, oracle.batch_init_feasible(3, p0, p1, p2))
