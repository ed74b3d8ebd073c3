"""The derivative restatements away from the default problems, without a GPU: non-zero end velocities (the
reference's special keys change vel0 and vel2), unsolved states, acceleration limits other than 100, and constraint pairs with
multipliers of exactly 0 or so small that D_j^2 underflows.  First the independent longdouble references are checked where they
will be used -- the oracle's kkt() against kkt_ld, the first derivatives against central differences of the oracle's solve at fixed
end velocities, the second derivatives against differences of the longdouble Jacobian at re-solved states -- then the kernels'
float64 / double-double restatements (tests/sensitivity_jvp_ref.py, tests/sensitivity_hess_ref.py) against them.

The end-velocity family: the feasible start of the generators' problems with vel0 = s U(-1, 1) t0 and vel2 = s U(-1, 1) t1 (t0, t1
the start's durations), solved by the oracle.  Without end velocities no generator produces an optimum with two or three active
constraints whose active rows leave a null space; with them more than half of the non-monotone problems end there, and a K
condensed in float64 lost the solution's null-space component (Jacobian errors up to 1e2 relative at gap 1e-13)."""
import numpy as np
import pytest

import sensitivity_hess_ref as hr
import sensitivity_jvp_ref as jr
import sensitivity_ref as sr

LD = np.longdouble
DISTS = [0, 1, 2]
DIST_IDS = ["monotone", "reference_like", "non_monotone"]
L_DEFAULT = 100.0


def end_velocity_family(orc, dist, s, gap_tol, n=1024, seed=21):
    """(positions (3 arrays), oracle-solved states) of the end-velocity family."""
    p = orc.gen_problems(seed, 0, n, dist)
    st = orc.batch_init_feasible(3, *p)
    rng = np.random.default_rng(seed)
    st[:, 12] = s * rng.uniform(-1, 1, n) * st[:, 1]
    st[:, 15] = s * rng.uniform(-1, 1, n) * st[:, 2]
    orc.batch_solve_gated(3, st, gap_tol, 200)
    return p, st


def edge_state(n, pair, lam, seed=0):
    """n feasible states around positions 0 / 200 / 400, vel1 57, durations 3.5 / 3.5, every multiplier 0.01 but the two of
    constraint pair `pair`, which are `lam` (0, or so small that D_j^2 underflows)."""
    rng = np.random.default_rng(seed)
    st = np.zeros((n, 16))
    st[:, 0] = 57 + rng.uniform(-2, 2, n)
    st[:, 1] = 3.5 + rng.uniform(-0.05, 0.05, n)
    st[:, 2] = 3.5 + rng.uniform(-0.05, 0.05, n)
    st[:, 3:11] = 0.01
    st[:, 3 + 2 * pair] = st[:, 4 + 2 * pair] = lam
    st[:, 13] = 200 + rng.uniform(-5, 5, n)
    st[:, 14] = 400 + rng.uniform(-5, 5, n)
    return st


def scaled_states(states, limit):
    """The central-path points at acceleration limit `limit` with the same perturbation p: positions, velocities and accelerations
    scale with the limit, durations do not, multipliers scale inversely (lam_i c_i is unchanged).  Exact up to rounding; the
    caller polishes them with resolve_ld."""
    k = limit / L_DEFAULT
    s = np.array(states, dtype=np.float64)
    s[:, [0, 11, 12, 13, 14, 15]] *= k
    s[:, 3:11] /= k
    return s


def _rel(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _longdouble(states, limit=L_DEFAULT):
    J, H = hr.full_hessian(states, M=hr.kkt_ld(states, limit), limit=limit)
    return J.astype(np.float64), H.astype(np.float64)


def restatement_errors(states, limit=L_DEFAULT, seed=0):
    """Normwise relative errors per problem of the four restatements against the longdouble 11 x 11 solve, on the rows the NaN rule
    keeps: dict of arrays, and the mask of rows NaN by the rule."""
    n = len(states)
    rng = np.random.default_rng(seed)
    g, td = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    vjp, jvp = jr.condensed_vjp(states, g, limit), jr.condensed_jvp(states, td, limit)
    J = jr.condensed_jacobian(states, limit)
    Jh, H = hr.condensed_hessian(states, limit)
    ok = jr.condensed(states, limit)["ok"]
    for x in (vjp, jvp, J, Jh, H):
        assert np.array_equal(np.all(np.isfinite(x.reshape(n, -1)), axis=1), ok)
    Jf, Hf = _longdouble(states[ok], limit)
    err = dict(vjp=_rel(vjp[ok], np.einsum("na,nab->nb", g[ok], Jf)), jvp=_rel(jvp[ok], np.einsum("nab,nb->na", Jf, td[ok])),
               jac=np.maximum(_rel(J[ok], Jf), _rel(Jh[ok], Jf)), hess=_rel(H[ok], Hf))
    return err, ~ok


def rounding_infeasible(states, limit=L_DEFAULT):
    """Rows whose largest constraint value, in the kernels' arithmetic, is positive by no more than rounding of a - L."""
    cmax = jr.condensed(states, limit)["cmax"]
    return (cmax > 0) & (cmax <= 64 * np.finfo(np.float64).eps * limit)


# Measured (1024 problems per row, seed 21; the float64 K of the parent revision in brackets), worst normwise relative error:
#                                   first-order entries           Hessian
#   monotone / reference-like       <= 3.1e-15                    <= 5.1e-11 (1 problem; 99.9 % <= 3e-15)
#   non-monotone, s = 0.02, 1e-8    1.0e-13  [6.2e-2]             1.8e-9   [7.7e-3]
#   non-monotone, s = 0.02, 1e-13   7.1e-13  [1.3e+2]             1.8e-10  [7.8e+1]
#   non-monotone, s = 0.1           <= 6.8e-13                    <= 2.2e-9
# 16384 problems per row: first order <= 4.6e-12, Hessian <= 3.9e-9.  On the device (tests/test_gpu_sensitivity_edges.py, 65,536
# problems of all three distributions per run, end velocities through set_state, nudge and field_ptr): first order <= 1.2e-11,
# Hessian <= 3.7e-8 (the parent revision's kernels: 0.43 and 0.67).  The Hessian's worst rows are those whose own first-order 7 x 7
# solve meets cond(M) ~ 1e8; the parent's form has the same error there.  Bounds: ~5-10x the worst.
def end_velocity_bound(gap_tol):
    """(first-order, Hessian) bounds for the end-velocity family, the device's 65,536-problem runs included."""
    return 1e-10, 2e-7


@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_kkt_ld_is_the_oracles_matrix_with_end_velocities(oracle, dist):
    for s, gap in ((0.02, 1e-8), (0.1, 1e-13)):
        _, st = end_velocity_family(oracle, dist, s, gap, n=256)
        assert np.any(st[:, 12] != 0) and np.any(st[:, 15] != 0)
        Mo = sr.kkt_batch(oracle, st)
        Ml = hr.kkt_ld(st).astype(np.float64)
        err = np.max(np.abs(Mo - Ml), axis=(1, 2)) / np.max(np.abs(Mo), axis=(1, 2))
        print("dist %d s %g: |kkt - kkt_ld| %.2e" % (dist, s, err.max()))
        assert err.max() <= 1e-14


@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_first_order_references_match_oracle_differences(oracle, dist):
    # the longdouble Jacobian (Oracle.kkt, and kkt_ld) against central differences of the oracle's solve with the end velocities held
    n, s = 512, 0.05
    p, base = end_velocity_family(oracle, dist, s, 1e-13, n=n, seed=22)
    v0, v2 = base[:, 12].copy(), base[:, 15].copy()
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1]))
    act = lambda x: x[:, 3:11] > 1e-6      # noqa: E731
    fd = np.zeros((n, 3, 3))
    stable = np.ones(n, dtype=bool)
    for b in range(3):
        sides = []
        for sgn in (1, -1):
            q = [x.copy() for x in p]
            q[b] = q[b] + sgn * h
            st = oracle.batch_init_feasible(3, *q)
            st[:, 12], st[:, 15] = v0, v2
            oracle.batch_solve_gated(3, st, 1e-13, 200)
            sides.append(st)
            stable &= np.all(act(st) == act(base), axis=1)
        fd[:, :, b] = (sides[0][:, :3] - sides[1][:, :3]) / (2 * h[:, None])
    J = sr.jacobian(oracle, base).astype(np.float64)
    Jl, _ = _longdouble(base)
    err = _rel(J[stable], fd[stable])
    print("dist %d: %d of %d active-set-stable, |J - fd| median %.2e 99 %% %.2e worst %.2e; oracle kkt vs kkt_ld Jacobian %.2e"
          % (dist, stable.sum(), n, np.median(err), np.percentile(err, 99), err.max(), _rel(J, Jl).max()))
    # measured: median <= 8.9e-9; 99 % 9.3e-7 / 3.4e-7 / 2.6e-5, worst 2.0e-6 / 4.2e-7 / 1.3e-4 (monotone / reference-like /
    # non-monotone: the tail sits next to changes of active set, where the O(h^2) truncation is large).  The fixed-p differences of
    # test_second_order_reference_matches_resolved_differences check the non-monotone problems tightly.
    assert stable.mean() > 0.8 and np.median(err) <= 1e-7 and np.percentile(err, 99) <= (1e-5 if dist < 2 else 1e-4)
    assert err.max() <= 1e-3
    assert _rel(J, Jl).max() <= 1e-12
    g = np.random.default_rng(1).standard_normal((n, 3))
    assert _rel(sr.vjp(oracle, base, g).astype(np.float64), np.einsum("na,nab->nb", g, J)).max() <= 1e-13
    assert _rel(jr.full_jvp(oracle, base, g).astype(np.float64), np.einsum("nab,nb->na", J, g)).max() <= 1e-13


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_second_order_reference_matches_resolved_differences(oracle, dist, gap_tol):
    # full_hessian against central differences of the longdouble Jacobian at states re-solved (resolve_ld) at fixed p
    n = 128
    p, states = end_velocity_family(oracle, dist, 0.05, gap_tol, n=n, seed=23)
    pp = np.array([oracle.kkt(3, s)[2] for s in states])
    pos = np.stack(p, axis=1)
    z, res = hr.resolve_ld(states, pp, pos)
    assert res.max() <= 1e-15
    M = hr.kkt_ld(z)
    J, H = hr.full_hessian(z, M=M)
    zu = hr.first_order(M, z)
    h = LD(1e-6) * np.maximum(np.abs(pos[:, 1] - pos[:, 0]), np.abs(pos[:, 2] - pos[:, 1])).astype(LD)
    err, err_j = np.zeros(n), np.zeros(n)
    for b in range(3):
        zb = sum(hr.P[u][b] * zu[:, u] for u in range(2))
        Js, xs = [], []
        for sgn in (1, -1):
            q = pos.astype(LD)
            q[:, b] += sgn * h
            start = z.copy()
            start[:, :11] += sgn * h[:, None] * zb
            zz, r = hr.resolve_ld(start, pp, q)
            assert r.max() <= 1e-15
            Js.append(hr.full_hessian(zz, M=hr.kkt_ld(zz))[0])
            xs.append(zz[:, :3])
        fd = (Js[0] - Js[1]) / (2 * h[:, None, None])
        fx = (xs[0] - xs[1]) / (2 * h[:, None])
        err_j = np.maximum(err_j, np.max(np.abs((fx - J[:, :, b]).astype(np.float64)), axis=1) / np.max(np.abs(J.astype(np.float64)), axis=(1, 2)))
        e = np.max(np.abs((fd - H[:, :, :, b]).astype(np.float64)), axis=(1, 2)) / np.max(np.abs(H.astype(np.float64)), axis=(1, 2, 3))
        err = np.maximum(err, e)
    print("dist %d gap %g: longdouble Jacobian vs differences of x: worst %.2e; Hessian vs differences of the Jacobian: median %.2e, "
          "worst %.2e" % (dist, gap_tol, err_j.max(), np.median(err), err.max()))
    # measured (relative to max |J|, max |H|; the O(h^2) truncation): Jacobian worst 1.3e-10 / 3.1e-11 / 6.8e-9, Hessian median
    # <= 1.6e-11, worst 6.6e-10 / 1.5e-10 / 3.4e-8 (monotone / reference-like / non-monotone, both gaps)
    assert err_j.max() <= (1e-9 if dist < 2 else 5e-8) and err.max() <= (1e-8 if dist < 2 else 3e-7)


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("s", [0.02, 0.1])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_restatements_with_end_velocities(oracle, dist, s, gap_tol):
    _, st = end_velocity_family(oracle, dist, s, gap_tol)
    err, nan = restatement_errors(st)
    first = max(err["vjp"].max(), err["jvp"].max(), err["jac"].max())
    print("dist %d s %g gap %g: first order worst %.2e (VJP %.2e JVP %.2e Jacobian %.2e), Hessian worst %.2e 99.9 %% %.2e; %d NaN rows"
          % (dist, s, gap_tol, first, err["vjp"].max(), err["jvp"].max(), err["jac"].max(), err["hess"].max(),
             np.percentile(err["hess"], 99.9), nan.sum()))
    # NaN only where an active constraint's value rounds to just above 0 in the kernels' arithmetic (the oracle's own rounding
    # calls the state feasible): the NaN rule, not the form
    assert nan.sum() <= 4 and np.all(rounding_infeasible(st[nan]))
    bj, bh = end_velocity_bound(gap_tol)
    assert first <= bj and err["hess"].max() <= bh


def _unsolved(orc, dist, n=1024, seed=24):
    """(label, states): the feasible start, 1, 3 and 8 fixed steps from it."""
    p = orc.gen_problems(seed, 0, n, dist)
    st = orc.batch_init_feasible(3, *p)
    out, done = [("start", st.copy())], 0
    for k in (1, 3, 8):
        orc.batch_steps(3, st, k - done)
        done = k
        out.append(("%d steps" % k, st.copy()))
    return out


# Measured, worst normwise relative error (first order / Hessian):
#   unsolved: the feasible start and 1, 3, 8 fixed steps (1024 problems per distribution, seed 24)    6.9e-13 / 1.2e-12
#   init_default, init_stuck and 1..8 steps from them                                                 2.5e-11 / 7.7e-11
#     (init_stuck's states have cond(M) ~ 1e8 - 7e9; from init_default the symmetric problem heads for a degenerate optimum, cond(M)
#      1e14 after 20 steps, where both forms carry cond(M) eps)
#   other limits: 37.5 and 250, gaps 1e-8 and 1e-11 (512 problems per distribution)                   1.4e-13 / 3.6e-10
#   edge multipliers: one pair at 0 or 1e-170 (256 states per case)                                   2.9e-15 / 1.1e-14
#     (on the device, 4,096 states per case: 4.5e-14 / 1.3e-14; the parent revision's Hessian was NaN)
# Bounds: ~5-10x ("default": the end-velocity bounds).
EDGE_BOUND = {"unsolved": (1e-11, 1e-11), "init": (3e-10, 1e-9), "default": (1e-10, 2e-7), "edge": (3e-13, 1e-13)}


@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_restatements_on_unsolved_states(oracle, dist):
    worst = np.zeros(2)
    for label, st in _unsolved(oracle, dist):
        err, nan = restatement_errors(st)
        assert nan.sum() == 0, label
        first = max(err["vjp"].max(), err["jvp"].max(), err["jac"].max())
        print("dist %d %s: first order worst %.2e, Hessian worst %.2e" % (dist, label, first, err["hess"].max()))
        worst = np.maximum(worst, (first, err["hess"].max()))
    assert worst[0] <= EDGE_BOUND["unsolved"][0] and worst[1] <= EDGE_BOUND["unsolved"][1]


def test_restatements_at_init_default_and_init_stuck(oracle):
    for init in (oracle.init_default(3), oracle.init_stuck()):
        st = np.tile(init, (9, 1))
        for k in range(1, 9):
            oracle.batch_steps(3, st[k:k + 1], k)
        err, nan = restatement_errors(st)
        first = max(err["vjp"].max(), err["jvp"].max(), err["jac"].max())
        print("0..8 steps: first order worst %.2e, Hessian worst %.2e, %d NaN" % (first, err["hess"].max(), nan.sum()))
        assert nan.sum() == 0
        assert first <= EDGE_BOUND["init"][0] and err["hess"].max() <= EDGE_BOUND["init"][1]


@pytest.mark.parametrize("limit", [37.5, 250.0])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_restatements_at_other_limits(oracle, dist, limit):
    for gap in (1e-8, 1e-11):
        _, st = end_velocity_family(oracle, dist, 0.0, gap, n=512, seed=25)
        pp = np.array([oracle.kkt(3, s)[2] for s in st])
        scaled = scaled_states(st, limit)
        z, res = hr.resolve_ld(scaled, pp, scaled[:, [11, 13, 14]], limit=limit, iters=3)
        assert res.max() <= 1e-15 * limit
        z = z.astype(np.float64)
        err, nan = restatement_errors(z, limit)
        first = max(err["vjp"].max(), err["jvp"].max(), err["jac"].max())
        print("dist %d limit %g gap %g: first order worst %.2e, Hessian worst %.2e, %d NaN"
              % (dist, limit, gap, first, err["hess"].max(), nan.sum()))
        # rounded to float64, a re-solved state's active c_i can land just above 0: the NaN rule's rows
        assert nan.mean() <= 0.02 and np.all(rounding_infeasible(z[nan], limit))
        assert first <= EDGE_BOUND["default"][0] and err["hess"].max() <= EDGE_BOUND["default"][1]


@pytest.mark.parametrize("lam", [0.0, 1e-170])
@pytest.mark.parametrize("pair", [0, 1, 2, 3])
def test_restatements_with_edge_multipliers(pair, lam):
    st = edge_state(256, pair, lam, seed=pair)
    err, nan = restatement_errors(st)
    first = max(err["vjp"].max(), err["jvp"].max(), err["jac"].max())
    print("pair %d multipliers %g: first order worst %.2e, Hessian worst %.2e" % (pair, lam, first, err["hess"].max()))
    assert nan.sum() == 0      # finite, as the longdouble solve is: E_j / D_j^2 is not formed where D_j^2 is 0 or subnormal
    assert first <= EDGE_BOUND["edge"][0] and err["hess"].max() <= EDGE_BOUND["edge"][1]


def test_nan_rule_unchanged_next_to_edge_multipliers():
    st = edge_state(64, 0, 0.0)
    st[1::4, 5] = np.nan
    st[2::4, 0] = 1e3      # vel1 far outside the feasible set
    bad = np.zeros(64, dtype=bool)
    bad[1::4] = bad[2::4] = True
    _, H = hr.condensed_hessian(st)
    J = jr.condensed_jacobian(st)
    v = jr.condensed_vjp(st, np.ones((64, 3)))
    for x in (H, J, v):
        assert np.array_equal(np.all(np.isnan(x.reshape(64, -1)), axis=1), bad)
        assert np.all(np.isfinite(x[~bad]))
