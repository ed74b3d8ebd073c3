"""rp_batch_solution_jvp / rp_batch_solution_jacobian without a GPU: the ABI entries and the torch layer's input checks, and the
forward-mode math of DESIGN.md section 12 on the test-side restatements (tests/sensitivity_jvp_ref.py) -- the kernels' condensed
float64 form against a longdouble solve of the full 11 x 11 system, the identities, duality with the VJP restatement, and finite
differences of the oracle's solve."""
import os
import re

import numpy as np
import pytest

import sensitivity_jvp_ref as jr
import sensitivity_ref as sr
from test_sensitivity_cpu import IDENTITY_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048
DISTS = [0, 1, 2]
DIST_IDS = ["monotone", "reference_like", "non_monotone"]


def test_library_exports_jvp_and_jacobian_at_revision_7():
    import rocket_path_amd as rp
    from rocket_path_amd import capi
    lib = rp.load_library()
    text = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    for name in ("rp_batch_solution_jvp", "rp_batch_solution_jacobian"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and ("RP_API int %s(" % name) in text, name
    assert int(re.search(r"#define\s+RP_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    assert lib.rp_abi_version() == 7 and capi.ABI_VERSION == 7
    assert hasattr(rp.Batch, "solution_jvp") and hasattr(rp.Batch, "solution_jacobian")


def test_min_time_jacobian_rejects_cpu_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    import rocket_path_amd as rp
    from rocket_path_amd import autograd
    assert rp.min_time_jacobian is autograd.min_time_jacobian
    x = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        autograd.min_time_jacobian(x, x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        autograd.min_time_jacobian(np.zeros(4), x, x)


def test_min_time_solve_has_a_forward_mode_rule():
    pytest.importorskip("torch")
    from rocket_path_amd import autograd
    fn = autograd._MinTimeSolve
    # torch.func.jvp needs the setup_context form and a jvp staticmethod
    for name in ("setup_context", "jvp"):
        assert name in vars(fn), name


def _solved(orc, dist, gap_tol, seed=13):
    p = orc.gen_problems(seed, 0, N, dist)
    states, _ = sr.solved_states(orc, *p, gap_tol)
    return p, states


# Measured on these problems (2048 of each distribution, seed 13), normwise relative per problem, condensed float64 against the
# longdouble 11 x 11 solve:
#                     JVP median / 99.9 % / worst         Jacobian worst
#   monotone          5.6e-16 / 3.1e-14 / 5.1e-14         4.7e-15
#   reference-like    5.9e-16 / 1.7e-14 / 4.3e-14         2.7e-15
#   non-monotone      2.1e-14 / 2.0e-13 / 2.3e-13         2.4e-13
# (the worst of gaps 1e-8 and 1e-13; the two gaps measure alike).  Bounds: 4-5x the worst.
CONDENSED_BOUND = {0: 2e-13, 1: 2e-13, 2: 1e-12}


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_condensed_forward_solve_matches_longdouble(oracle, dist, gap_tol):
    p, states = _solved(oracle, dist, gap_tol)
    tdot = np.random.default_rng(3).standard_normal((N, 3))
    full = jr.full_jvp(oracle, states, tdot).astype(np.float64)
    con = jr.condensed_jvp(states, tdot)
    err = np.linalg.norm(con - full, axis=1) / np.linalg.norm(full, axis=1)
    Jc, Jf = jr.condensed_jacobian(states), jr.full_jacobian(oracle, states).astype(np.float64)
    err_j = np.linalg.norm(Jc - Jf, axis=(1, 2)) / np.linalg.norm(Jf, axis=(1, 2))
    print("dist %d gap %g: JVP median %.2e, 99.9 %% %.2e, worst %.2e; Jacobian worst %.2e"
          % (dist, gap_tol, np.median(err), np.percentile(err, 99.9), err.max(), err_j.max()))
    assert np.all(np.isfinite(con)) and np.all(np.isfinite(Jc))
    assert err.max() <= CONDENSED_BOUND[dist] and err_j.max() <= CONDENSED_BOUND[dist]


@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_equal_tangents_give_exactly_zero(oracle, dist):
    _, states = _solved(oracle, dist, 1e-8)
    t = np.random.default_rng(4).standard_normal(N)
    out = jr.condensed_jvp(states, np.stack([t, t, t], axis=1))
    assert np.all(out == 0)


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_homogeneity(oracle, dist, gap_tol):
    # theta_dot = theta: scaling the positions by s scales times and speeds by sqrt(s), so x_dot = x / 2 at the optimum
    p, states = _solved(oracle, dist, gap_tol)
    x = states[:, :3]
    out = jr.condensed_jvp(states, np.stack(p, axis=1))
    hom = np.max(np.abs(out - x / 2), axis=1) / np.max(np.abs(x), axis=1)
    print("dist %d gap %g: homogeneity %.2e" % (dist, gap_tol, hom.max()))
    assert hom.max() <= IDENTITY_BOUND[gap_tol]["hom"]


# g . (J theta_dot) against (J^T g) . theta_dot with the VJP's longdouble restatement, relative to |g| |x_dot|: measured worst
# 5.0e-14 (monotone, reference-like) and 1.9e-13 (non-monotone)
@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_duality_with_the_vjp_restatement(oracle, dist, gap_tol):
    _, states = _solved(oracle, dist, gap_tol)
    rng = np.random.default_rng(5)
    tdot, g = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    xdot = jr.condensed_jvp(states, tdot)
    lhs = np.sum(g * xdot, axis=1)
    rhs = np.sum(sr.vjp(oracle, states, g).astype(np.float64) * tdot, axis=1)
    err = np.abs(lhs - rhs) / (np.linalg.norm(g, axis=1) * np.linalg.norm(xdot, axis=1))
    print("dist %d gap %g: duality worst %.2e" % (dist, gap_tol, err.max()))
    assert err.max() <= 1e-12


@pytest.mark.parametrize("dist", [0, 1], ids=["monotone", "reference_like"])
def test_forward_solve_matches_finite_differences(oracle, dist):
    p = oracle.gen_problems(17, 0, N, dist)
    tdot = np.random.default_rng(6).standard_normal((N, 3))
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1])) / np.max(np.abs(tdot), axis=1)
    base, _ = sr.solved_states(oracle, *p, 1e-13)
    lo, _ = sr.solved_states(oracle, *[q - h * tdot[:, j] for j, q in enumerate(p)], 1e-13)
    hi, _ = sr.solved_states(oracle, *[q + h * tdot[:, j] for j, q in enumerate(p)], 1e-13)
    fd = (hi[:, :3] - lo[:, :3]) / (2 * h[:, None])
    act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
    ok = np.all((act(base) == act(lo)) & (act(base) == act(hi)), axis=1)
    xdot = jr.condensed_jvp(base, tdot)
    err = np.linalg.norm((xdot - fd)[ok], axis=1) / np.linalg.norm(xdot[ok], axis=1)
    print("dist %d: %d of %d active-set-stable, worst relative |x_dot - fd| %.2e" % (dist, ok.sum(), N, err.max()))
    assert ok.mean() > 0.9 and err.max() <= 1e-5
