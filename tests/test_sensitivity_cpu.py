"""rp_batch_solution_vjp without a GPU: the ABI entry and the torch layer's input checks, and the math of DESIGN.md section 12 on
the test-side restatement (tests/sensitivity_ref.py) -- against finite differences of the oracle's solve, and the identities that
follow from the problem's structure."""
import os
import re

import numpy as np
import pytest

import sensitivity_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048


def test_library_exports_vjp_and_agrees_on_revision_7():
    import rocket_path_amd as rp
    from rocket_path_amd import capi
    lib = rp.load_library()
    assert hasattr(lib, "rp_batch_solution_vjp") and "rp_batch_solution_vjp" in capi.SIGNATURES
    text = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    assert "rp_batch_solution_vjp" in text
    assert int(re.search(r"#define\s+RP_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    assert lib.rp_abi_version() == 7 and capi.ABI_VERSION == 7


def test_autograd_rejects_cpu_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    import rocket_path_amd as rp
    from rocket_path_amd import autograd
    assert rp.min_time_solve is autograd.min_time_solve
    x = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        autograd.min_time_solve(x, x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        autograd.min_time_solve(np.zeros(4), x, x)


def _problems(orc, dist, seed=11):
    return orc.gen_problems(seed, 0, N, dist)


def _stable(orc, states, lo, hi):
    """Problems whose active set (lambda_i > 1e-6) is the same at the state and both perturbed solves."""
    act = lambda s: s[:, 3:11] > 1e-6      # noqa: E731
    a = act(states)
    return np.all((a == act(lo)) & (a == act(hi)), axis=1)


def _fd_jacobian(orc, p, gap_tol, h):
    """Central differences of the oracle's gated solve: (n, 3, 3) and the mask of active-set-stable problems."""
    n = len(p[0])
    J = np.zeros((n, 3, 3))
    ok = np.ones(n, dtype=bool)
    base, _ = sr.solved_states(orc, *p, gap_tol)
    for j in range(3):
        lo_p = [q.copy() for q in p]
        hi_p = [q.copy() for q in p]
        lo_p[j] -= h
        hi_p[j] += h
        lo, _ = sr.solved_states(orc, *lo_p, gap_tol)
        hi, _ = sr.solved_states(orc, *hi_p, gap_tol)
        J[:, :, j] = (hi[:, :3] - lo[:, :3]) / (2 * h[:, None] if np.ndim(h) else 2 * h)
        ok &= _stable(orc, base, lo, hi)
    return base, J, ok


@pytest.mark.parametrize("dist", [0, 1], ids=["monotone", "reference_like"])
def test_restatement_matches_finite_differences(oracle, dist):
    p = _problems(oracle, dist)
    h = 1e-4 * np.maximum(np.abs(p[1] - p[0]), np.abs(p[2] - p[1]))
    states, J_fd, ok = _fd_jacobian(oracle, p, 1e-13, h)
    assert ok.mean() > 0.9
    J = sr.jacobian(oracle, states).astype(np.float64)
    err = np.linalg.norm((J - J_fd)[ok], axis=(1, 2)) / np.linalg.norm(J[ok], axis=(1, 2))
    print("dist %d: %d of %d active-set-stable, worst relative |J - J_fd| %.2e" % (dist, ok.sum(), N, err.max()))
    assert np.all(np.isfinite(J)) and err.max() <= 1e-5


# Measured on these problems (2048 of each distribution, seed 12), relative per problem:
#                     translation   homogeneity (worst)   envelope (median / 99.9 % / worst)
#   gap 1e-8          2e-16         1.2e-9                3.6e-10 / 1.8e-7 / 2.7e-5
#   gap 1e-13         2e-16         2.3e-14               5.4e-15 / 2.8e-12 / 4.5e-11
# The identities hold for the optimum; the central-path point the solve stops at is O(gap) away from it, and the envelope's
# relative error is largest where d(t0 + t1)/dtheta itself is small.  On bench.py's 1 Mi problems at gap 1e-8 (a float64 restatement
# of the kernel on the oracle's states): homogeneity 1.7e-9, envelope 3.5e-10 / 9.7e-7 / 2.5e-4.  The bounds asserted here and by
# the full-size GPU test (tests/test_gpu_sensitivity.py) cover both with a margin of 3-6x:
IDENTITY_BOUND = {1e-8: dict(hom=1e-8, env_999=3e-6, env=1e-3), 1e-13: dict(hom=1e-12, env_999=1e-10, env=1e-9)}


def identity_errors(orc, p, states, J):
    """(translation, homogeneity, envelope) relative errors per problem, from the Jacobian J (n, 3, 3) at `states`."""
    J = np.asarray(J, dtype=np.float64)
    pos = np.stack(p, axis=1)
    scale = np.max(np.abs(J), axis=(1, 2))
    trans = np.max(np.abs(J.sum(axis=2)), axis=1) / scale
    lhs = np.einsum("nkj,nj->nk", J, pos)
    x = states[:, :3]
    hom = np.max(np.abs(lhs - x / 2), axis=1) / np.max(np.abs(x), axis=1)
    total = J[:, 1, :] + J[:, 2, :]
    lam = states[:, 3:11]
    dc = sr.constraint_dtheta(states).astype(np.float64)
    env = np.max(np.abs(total - np.einsum("ni,nij->nj", lam, dc)), axis=1) / np.max(np.abs(total), axis=1)
    return trans, hom, env


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", [0, 1], ids=["monotone", "reference_like"])
def test_identities_on_the_restatement(oracle, dist, gap_tol):
    p = _problems(oracle, dist, seed=12)
    states, _ = sr.solved_states(oracle, *p, gap_tol)
    J = sr.jacobian(oracle, states)
    trans, hom, env = identity_errors(oracle, p, states, J)
    print("dist %d gap %g: translation %.2e homogeneity %.2e envelope %.2e" % (dist, gap_tol, trans.max(), hom.max(), env.max()))
    assert trans.max() <= 1e-12
    bound = IDENTITY_BOUND[gap_tol]
    assert hom.max() <= bound["hom"]
    assert np.percentile(env, 99.9) <= bound["env_999"] and env.max() <= bound["env"]
