"""rp_batch_solution_hessian and double backward without a GPU: the ABI entry, the torch layer's entry points, and the second-order
math of DESIGN.md section 12 on the test-side restatements (tests/sensitivity_hess_ref.py) -- the derivative tables against finite
differences, the longdouble definition against differences of its own Jacobian at re-solved states, the kernel's float64 form
against the longdouble one, the rejected naive form's dual steps, symmetry, translation and homogeneity."""
import os
import re

import numpy as np
import pytest

import sensitivity_hess_ref as hr
import sensitivity_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048
LD = np.longdouble
DISTS = [0, 1, 2]
DIST_IDS = ["monotone", "reference_like", "non_monotone"]


def test_library_exports_hessian_at_revision_7():
    import rocket_path_amd as rp
    from rocket_path_amd import autograd, capi
    lib = rp.load_library()
    text = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    name = "rp_batch_solution_hessian"
    assert hasattr(lib, name) and name in capi.SIGNATURES and ("RP_API int %s(" % name) in text
    assert int(re.search(r"#define\s+RP_ABI_VERSION\s+(\d+)", text).group(1)) == 7
    assert lib.rp_abi_version() == 7 and capi.ABI_VERSION == 7
    assert hasattr(rp.Batch, "solution_hessian")
    assert rp.min_time_hessian is autograd.min_time_hessian


def test_min_time_hessian_rejects_cpu_tensors_before_the_library():
    torch = pytest.importorskip("torch")
    from rocket_path_amd import autograd
    x = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        autograd.min_time_hessian(x, x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        autograd.min_time_hessian(np.zeros(4), x, x)


def test_min_time_solve_backward_is_differentiable():
    pytest.importorskip("torch")
    from rocket_path_amd import autograd
    # once_differentiable wraps the function it decorates (functools.wraps: __wrapped__): the backward of the solve must be the
    # plain one, and its own backward (_SolutionVJP) the once-differentiable one
    assert not hasattr(autograd._MinTimeSolve.backward, "__wrapped__")
    assert hasattr(autograd._SolutionVJP.backward, "__wrapped__")


def _solved(orc, dist, gap_tol, seed=13, n=N):
    p = orc.gen_problems(seed, 0, n, dist)
    states, _ = sr.solved_states(orc, *p, gap_tol)
    return p, states


@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_derivative_tables_match_finite_differences(oracle, dist):
    # every table entry against a longdouble central difference of the one below it, in v, t and dX of the pair's segment
    _, states = _solved(oracle, dist, 1e-8, n=256)
    s = np.asarray(states, dtype=LD)
    T = hr.accel_tables(s)
    eps = LD(1e-7)

    def moved(var, j, d):
        q = s.copy()
        seg = j >> 1
        if var == "v":
            q[:, 0] += d
        elif var == "t":
            q[:, 1 + seg] += d * q[:, 1 + seg]
        else:      # dX of the segment: move its end position
            q[:, 13 + seg] += d * np.abs(q[:, 13 + seg] - q[:, 11 + 2 * seg] + 1)
        return hr.accel_tables(q)

    def scale(var, j):
        seg = j >> 1
        return {"v": np.ones(len(s), dtype=LD), "t": s[:, 1 + seg], "X": np.abs(s[:, 13 + seg] - s[:, 11 + 2 * seg] + 1)}[var]
    worst = 0.0
    for key, (base, var) in {"v": ("a", "v"), "t": ("a", "t"), "X": ("a", "X"), "tt": ("t", "t"), "vt": ("v", "t"),
                             "Xt": ("X", "t"), "ttt": ("tt", "t"), "vtt": ("vt", "t"), "Xtt": ("Xt", "t")}.items():
        for j in range(4):
            hi, lo = moved(var, j, eps), moved(var, j, -eps)
            fd = (hi[base][:, j] - lo[base][:, j]) / (2 * eps * scale(var, j))
            err = np.abs(fd - T[key][:, j]) / np.maximum(np.abs(T[key][:, j]), np.abs(T[base][:, j]) / scale(var, j))
            worst = max(worst, float(err.max()))
    print("dist %d: derivative tables vs differences worst %.2e" % (dist, worst))
    assert worst <= 1e-9


def test_kkt_ld_is_the_oracles_matrix(oracle):
    _, states = _solved(oracle, 1, 1e-8, n=256)
    Mo = sr.kkt_batch(oracle, states)
    Ml = hr.kkt_ld(states).astype(np.float64)
    err = np.max(np.abs(Mo - Ml), axis=(1, 2)) / np.max(np.abs(Mo), axis=(1, 2))
    assert err.max() <= 1e-14


# Measured (256 problems each, seed 19, gap 1e-8, h = 1e-6 |dX|): central differences of the longdouble Jacobian at states re-solved
# to |r| ~ 1e-18 at fixed p against the longdouble Hessian: median 2e-12 / 5e-12, worst 6.7e-10 / 1.8e-10 (monotone / reference-like),
# relative to max |H| -- the O(h^2) truncation.
@pytest.mark.parametrize("dist", [0, 1], ids=["monotone", "reference_like"])
def test_full_hessian_matches_differences_at_resolved_states(oracle, dist):
    n = 256
    p, states = _solved(oracle, dist, 1e-8, seed=19, n=n)
    pp = np.array([oracle.kkt(3, s)[2] for s in states])      # the perturbation the next step would use, held fixed
    pos = np.stack(p, axis=1)
    z, res = hr.resolve_ld(states, pp, pos)
    assert res.max() <= 1e-16
    M = hr.kkt_ld(z)
    _, H = hr.full_hessian(z, M=M)
    zu = hr.first_order(M, z)
    h = LD(1e-6) * np.maximum(np.abs(pos[:, 1] - pos[:, 0]), np.abs(pos[:, 2] - pos[:, 1])).astype(LD)
    err = np.zeros(n)
    for b in range(3):
        zb = sum(hr.P[u][b] * zu[:, u] for u in range(2))      # first-order predictor along pos_b
        Js = []
        for sgn in (1, -1):
            q = pos.astype(LD)
            q[:, b] += sgn * h
            start = z.copy()
            start[:, :11] += sgn * h[:, None] * zb
            zz, r = hr.resolve_ld(start, pp, q)
            assert r.max() <= 1e-16
            Js.append(hr.full_hessian(zz, M=hr.kkt_ld(zz))[0])
        fd = (Js[0] - Js[1]) / (2 * h[:, None, None])
        e = np.max(np.abs((fd - H[:, :, :, b]).astype(np.float64)), axis=(1, 2)) / np.max(np.abs(H.astype(np.float64)), axis=(1, 2, 3))
        err = np.maximum(err, e)
    print("dist %d: longdouble Hessian vs differences of the Jacobian: median %.2e, worst %.2e" % (dist, np.median(err), err.max()))
    assert err.max() <= 1e-8


def _rel(a, b):
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


# Measured on these problems (2048 of each distribution, seed 13), normwise relative per problem against the longdouble 11 x 11
# solve, the worst of gaps 1e-8 and 1e-13:
#                     chosen form (7 x 7 first order)       naive form (mu_u = D A_u from K)
#                     H median / worst     J worst          H median / worst
#   monotone          7.9e-16 / 2.9e-14    7.6e-16          1.1e-15 / 6.9e-14
#   reference-like    7.8e-16 / 4.3e-15    7.7e-16          9.9e-16 / 1.5e-14
#   non-monotone      3.0e-14 / 2.5e-13    2.1e-14          3.4e-14 / 2.5e-13
# Bounds: 4-7x the worst.
CONDENSED_BOUND = {0: 2e-13, 1: 2e-13, 2: 1e-12}


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_condensed_hessian_matches_longdouble(oracle, dist, gap_tol):
    _, states = _solved(oracle, dist, gap_tol)
    Jf, Hf = hr.full_hessian(states, orc=oracle)
    Jf, Hf = Jf.astype(np.float64), Hf.astype(np.float64)
    Jc, Hc = hr.condensed_hessian(states)
    _, Hn = hr.naive_hessian(states)
    err, err_j, err_n = _rel(Hc, Hf), _rel(Jc, Jf), _rel(Hn, Hf)
    print("dist %d gap %g: Hessian median %.2e, 99.9 %% %.2e, worst %.2e; Jacobian worst %.2e; naive form median %.2e, worst %.2e"
          % (dist, gap_tol, np.median(err), np.percentile(err, 99.9), err.max(), err_j.max(), np.median(err_n), err_n.max()))
    assert np.all(np.isfinite(Hc)) and np.all(np.isfinite(Jc))
    assert err.max() <= CONDENSED_BOUND[dist] and err_j.max() <= CONDENSED_BOUND[dist]


# The first-order dual steps mu_j,u themselves, against the longdouble solve's lam_p,u - lam_m,u (relative to the largest):
#                     chosen form: worst               naive form (D_j A_j,u): median / worst
#   gap 1e-8          7.6e-15 (non-monotone 6.8e-7)     2e-6 / 1.9e-5
#   gap 1e-13         2.8e-15 (non-monotone 4.0e-2)     0.18 / 4.4
# The naive form loses every digit at gap 1e-13: A_j,u cancels to O(p) on an active pair and its rounding comes back times D_j (up
# to 4e11 here).  The Hessian survives it because K^-1 h_j is O(1 / D_j) for an active pair, but nothing else built on mu_u would.
# The non-monotone optima are degenerate (4 active constraints for 3 unknowns), where the dual step is ill-determined.
@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_dual_steps_chosen_and_naive_forms(oracle, dist, gap_tol):
    _, states = _solved(oracle, dist, gap_tol)
    zu = hr.first_order(sr.kkt_batch(oracle, states), states)
    ref = (zu[:, :, 4::2] - zu[:, :, 3::2]).astype(np.float64)
    c = hr._pair_terms(states, hr.L_DEFAULT)
    _, mu_aware = hr.aware_first_order(c)
    _, mu_naive = hr.naive_dual_steps(c)
    sc = np.max(np.abs(ref), axis=(1, 2))
    ea = np.max(np.abs(mu_aware - ref), axis=(1, 2)) / sc
    en = np.max(np.abs(mu_naive - ref), axis=(1, 2)) / sc
    print("dist %d gap %g: dual steps, chosen form median %.2e worst %.2e; naive form median %.2e worst %.2e"
          % (dist, gap_tol, np.median(ea), ea.max(), np.median(en), en.max()))
    if dist < 2:
        assert ea.max() <= 1e-13
        assert en.max() >= (1e-7 if gap_tol == 1e-8 else 1e-2)      # why the naive form is not used
    else:
        assert ea.max() <= (1e-5 if gap_tol == 1e-8 else 0.2)


# Measured on the restatement (2048 problems each, seed 13), relative per problem:
#   sum_c H_a[b][c] pos_c = -J_a[b] / 2 (to max |J|)    pos^T H_a pos = -x_a / 4 (to max |x|)
#   gap 1e-8:  5.0e-10 / 2.5e-10 / 3.3e-10              6.2e-10 / 4.2e-10 / 4.2e-9       (monotone / reference-like / non-monotone)
#   gap 1e-13: 7.2e-15 / 2.9e-15 / 1.3e-13              4.8e-13 / 1.9e-14 / 2.9e-10
# Translation (row sums to max |H|): 1.1e-16.  The identities hold for the optimum; the returned point is O(gap) away from it.
HOM_BOUND = {1e-8: {0: (5e-9, 5e-9), 1: (5e-9, 5e-9), 2: (5e-9, 3e-8)},
             1e-13: {0: (1e-13, 5e-12), 1: (1e-13, 5e-12), 2: (1e-12, 3e-9)}}


@pytest.mark.parametrize("gap_tol", [1e-8, 1e-13])
@pytest.mark.parametrize("dist", DISTS, ids=DIST_IDS)
def test_symmetry_translation_and_homogeneity(oracle, dist, gap_tol):
    p, states = _solved(oracle, dist, gap_tol)
    J, H = hr.condensed_hessian(states)
    assert np.array_equal(H, np.swapaxes(H, 2, 3))
    tr = np.max(np.abs(H.sum(axis=3)), axis=(1, 2)) / np.max(np.abs(H), axis=(1, 2, 3))
    pos = np.stack(p, axis=1)
    x = states[:, :3]
    h1 = np.max(np.abs(np.einsum("nabc,nc->nab", H, pos) + J / 2), axis=(1, 2)) / np.max(np.abs(J), axis=(1, 2))
    h2 = np.max(np.abs(np.einsum("nb,nabc,nc->na", pos, H, pos) + x / 4), axis=1) / np.max(np.abs(x), axis=1)
    print("dist %d gap %g: translation %.2e, H pos + J/2 %.2e, pos H pos + x/4 %.2e" % (dist, gap_tol, tr.max(), h1.max(), h2.max()))
    assert tr.max() <= 1e-14
    b1, b2 = HOM_BOUND[gap_tol][dist]
    assert h1.max() <= b1 and h2.max() <= b2
