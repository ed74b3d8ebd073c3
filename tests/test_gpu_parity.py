"""Parity of the HIP path (through the C ABI) against the oracle and the golden fixtures.

Tolerances (BASELINE.json north_star): converged (duration, velocity) within 1e-10 relative,
identical iteration counts.  "Relative" is scale-aware, |d| <= tol * max(|x|, 1), because
non-monotone problems converge to vel1 ~ 1e-13 where a plain ratio is meaningless
(SURVEY.md section 7).  Golden data come from the restatement driven by the reference's own
Eigen QR (oracle/gen_golden.py); the live oracle uses its own Householder QR.
"""
import os
import subprocess

import numpy as np
import pytest

import rocket_path_amd as rp
from oracle_api import StepInfo
from parity_util import certify_iteration_counts, certify_line_search_decisions, keep_mask

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def serr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


LAM_TOL = 1e-9
# Non-monotone stress problems (mid position outside [start, end]) converge to vel1 ~ 1e-13 with two multipliers per segment
# sharing the load; there the multipliers themselves are ill-conditioned: the oracle with its own QR and the oracle with the
# reference's Eigen QR -- two CPU restatements that differ only in rounding order -- disagree by 5.0e-8 on them while
# agreeing to 4e-16 on the monotone and reference-like sets (tests/test_oracle_golden.py::test_multipliers_at_the_gate_...).
LAM_TOL_DEGENERATE = 2e-7


def lam_err(lam, ref):
    """Multipliers are compared per problem against that problem's largest multiplier: at the gate the active ones are
    O(1e-2..1) and the inactive ones O(gap / |c|) ~ 1e-10, so neither |x| nor max(|x|, 1) is a meaningful scale."""
    lam, ref = np.asarray(lam, dtype=float), np.asarray(ref, dtype=float)
    scale = np.max(np.abs(ref), axis=-1, keepdims=True)
    return float(np.max(np.abs(lam - ref) / scale))


@pytest.fixture(scope="module")
def g3(golden_dir):
    return np.load(os.path.join(golden_dir, "f3_batch.npz"))


@pytest.fixture(scope="module")
def traj(golden_dir):
    return np.load(os.path.join(golden_dir, "f3_trajectories.npz"))


# ---------------------------------------------------------------- config 1: the single default problem
def test_config1_default_problem_50_steps(traj):
    with rp.Batch(1) as b:
        b.init_default()
        s0 = b.get_state()[0]
        assert np.array_equal(s0[:11], traj["default_states"][0]) and np.array_equal(s0[11:], traj["default_const"])
        for s in range(1, 51):
            b.step(1)
            st = b.get_state()[0]
            assert np.all(np.isfinite(st)), s
            assert serr(st[:3], traj["default_states"][s, :3]) < TOL, s
            if s <= 20:   # multipliers too while they are above the noise floor
                assert serr(st[3:11], traj["default_states"][s, 3:11]) < 1e-9, s
        assert serr(st[:3], [200.0, 2.0, 2.0]) < 1e-13
        it, status = b.get_iters()
        assert it[0] == 50


def test_fused_steps_equal_single_steps_bitwise(g3):
    n = 1024
    init = g3["init"][:n]
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_state(init)
        b.set_state(init)
        a.step(7)
        for _ in range(7):
            b.step(1)
        assert np.array_equal(a.get_state(), b.get_state())


# ---------------------------------------------------------------- golden batch, fixed steps (config 2 shape)
def test_fixed_steps_against_golden(g3):
    n = len(g3["init"])
    with rp.Batch(n) as b:
        b.set_state(g3["init"])
        assert np.array_equal(b.get_state(), g3["init"])          # AoS -> SoA -> AoS is lossless in f64
        b.step(1)
        assert serr(b.get_state()[:, :3], g3["after1"][:, :3]) < TOL
        b.step(4)
        assert serr(b.get_state()[:, :3], g3["after5"][:, :3]) < TOL
        b.step(45)
        st = b.get_state()
        assert np.all(np.isfinite(st))
        assert serr(st[:, :3], g3["after50"][:, :3]) < TOL
        # ... and the multipliers after 50 steps (the reference's post-convergence regime: the point is frozen, every step
        # still walks ~48 residual halvings), relative to the problem's largest multiplier.  Pinned on the monotone and
        # reference-like sets.  On the non-monotone stress set the optimum has FOUR active constraints for three variables
        # (vel1 -> 0: both segments are bang-bang), so the multipliers have a null direction along which 35 post-convergence
        # steps drift freely: the oracle with its own QR and the reference (Eigen QR) -- two CPU evaluations of the same
        # algorithm -- differ by 0.42 of the largest multiplier there (median 8e-7; tests/test_oracle_golden.py), so no
        # tolerance is meaningful and only finiteness / sign are asserted.
        regular = g3["dist"] != rp.problems.DIST_NON_MONOTONE
        e_reg, e_deg = lam_err(st[regular, 3:11], g3["after50"][regular, 3:11]), lam_err(st[~regular, 3:11], g3["after50"][~regular, 3:11])
        print("multipliers after 50 fixed steps: %.2e (monotone / reference-like), %.2e (non-monotone: not determined)" % (e_reg, e_deg))
        assert e_reg < LAM_TOL
        assert np.all(st[:, 3:11] > 0)


def test_set_problems_applies_the_feasible_start_rule(g3):
    pos = g3["pos"]
    with rp.Batch(len(pos)) as b:
        b.set_problems(pos[:, 0], pos[:, 1], pos[:, 2])
        st = b.get_state()
        assert np.array_equal(st[:, 11:], g3["init"][:, 11:])
        assert np.array_equal(st[:, [0, 3, 4, 5, 6, 7, 8, 9, 10]], g3["init"][:, [0, 3, 4, 5, 6, 7, 8, 9, 10]])
        assert serr(st[:, 1:3], g3["init"][:, 1:3]) < 4e-16         # device sqrt/div vs libm: last-bit only


# ---------------------------------------------------------------- golden batch, gated (config 3 shape)
@pytest.mark.parametrize("steps_per_launch", [0, 1, 4])
def test_gated_solve_against_golden(g3, steps_per_launch):
    n = len(g3["init"])
    with rp.Batch(n) as b:
        b.set_state(g3["init"])
        b.solve(1e-8, 200, steps_per_launch)
        b.sync()
        it, status = b.get_iters()
        st = b.get_state()
        assert np.array_equal(it, g3["iters"])                      # identical iteration counts (no gate tie in this set)
        assert serr(st[:, :3], g3["gated"][:, :3]) < TOL
        regular = g3["dist"] != rp.problems.DIST_NON_MONOTONE         # the multipliers at the gate too
        assert lam_err(st[regular, 3:11], g3["gated"][regular, 3:11]) < LAM_TOL
        assert lam_err(st[~regular, 3:11], g3["gated"][~regular, 3:11]) < LAM_TOL_DEGENERATE
        assert np.array_equal(st[:, 11:], g3["init"][:, 11:])
        assert np.all(status == rp.ST_CONVERGED)
        r = b.reduce()
        assert r["n_converged"] == n and r["total_steps"] == float(g3["iters"].sum())
        assert r["max_gap"] < 1e-8


def test_fused_and_per_launch_solves_are_bitwise_identical(g3):
    n = 2048
    with rp.Batch(n) as a, rp.Batch(n) as b, rp.Batch(n) as c:
        for x in (a, b, c):
            x.set_state(g3["init"][:n])
        a.solve(1e-8, 200, 0)
        b.solve(1e-8, 200, 1)
        c.solve(1e-8, 200, 5)
        sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
        assert np.array_equal(sa, sb) and np.array_equal(sa, sc)
        assert np.array_equal(a.get_iters()[0], b.get_iters()[0]) and np.array_equal(a.get_iters()[0], c.get_iters()[0])


def test_solve_is_idempotent_and_respects_max_iter(g3):
    n = 512
    with rp.Batch(n) as b:
        b.set_state(g3["init"][:n])
        b.solve(1e-8, 3, 0)
        it, status = b.get_iters()
        assert np.all(it == 3) and np.all(status & rp.ST_MAXITER)
        st3 = b.get_state()
        b.solve(1e-8, 3, 0)                       # capped problems do not move again
        assert np.array_equal(b.get_state(), st3)
        b.set_state(g3["init"][:n])
        b.solve(1e-8, 200, 0)
        done = b.get_state()
        b.solve(1e-8, 200, 0)                     # converged problems do not move again
        assert np.array_equal(b.get_state(), done)
        assert np.array_equal(b.get_iters()[0], g3["iters"][:n])


# ---------------------------------------------------------------- live oracle on fresh seeds
@pytest.mark.parametrize("dist", [rp.problems.DIST_MONOTONE, rp.problems.DIST_REFERENCE_LIKE, rp.problems.DIST_NON_MONOTONE])
def test_gated_solve_against_live_oracle(oracle, dist):
    n = 20000
    p0, p1, p2 = rp.problems.generate(777, 0, n, dist)
    init = oracle.batch_init_feasible(3, p0, p1, p2)
    aos = init.copy()
    it_o, total = oracle.batch_solve_gated(3, aos, 1e-8, 200)
    with rp.Batch(n) as b:
        b.set_problems(p0, p1, p2)
        b.solve(1e-8, 200, 0)
        it_g, status = b.get_iters()
        st = b.get_state()
    ok = keep_mask(n, certify_iteration_counts(oracle, 3, init, it_g, it_o, 1e-8))      # identical, gate ties certified
    assert serr(st[ok, :3], aos[ok, :3]) < TOL
    assert lam_err(st[ok, 3:11], aos[ok, 3:11]) < (LAM_TOL_DEGENERATE if dist == rp.problems.DIST_NON_MONOTONE else LAM_TOL)
    assert np.all(status == rp.ST_CONVERGED)


# ---------------------------------------------------------------- edge cases
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000])
def test_ragged_batch_sizes(oracle, n):
    p0, p1, p2 = rp.problems.generate(5, 0, n, 0)
    aos = oracle.batch_init_feasible(3, p0, p1, p2)
    oracle.batch_steps(3, aos, 6)
    with rp.Batch(n) as b:
        b.set_problems(p0, p1, p2)
        b.step(6)
        assert serr(b.get_state()[:, :3], aos[:, :3]) < TOL


def test_stuck_state_trajectory(traj, oracle):
    with rp.Batch(3) as b:
        b.init_stuck()
        for s in range(1, 31):
            b.step(1)
            st = b.get_state()
            assert np.array_equal(st[0], st[1]) and np.array_equal(st[0], st[2])
            if s <= 12:
                assert serr(st[0, :3], traj["stuck_states"][s, :3]) < 1e-8, s
        # the method stalls here (initStuck, onedpath_ip.cpp:177-199): gap stays ~2.08
        assert abs(oracle.gap(3, st[0]) - 2.077) < 5e-3


def test_infeasible_start_is_frozen_and_flagged(traj):
    with rp.Batch(2) as b:
        b.init_default()
        b.nudge(13, 150.0)           # pos1 200 -> 350: SURVEY.md 8c's infeasible start (Up key x15)
        before = b.get_state()
        assert np.array_equal(before[0, 11:], traj["infeasible_const"])
        b.step(3)
        after = b.get_state()
        assert np.max(np.abs(after - before)) < 1e-25              # 100 halvings: s ~ 8e-31
        assert serr(after[0, :11], traj["infeasible_states"][3]) < 1e-12
        b.solve(1e-8, 5, 0)
        _, status = b.get_iters()
        assert np.all(status & rp.ST_INFEASIBLE) and np.all(status & rp.ST_MAXITER)


def test_non_finite_input_is_flagged_not_fatal():
    with rp.Batch(4) as b:
        b.init_default()
        st = b.get_state()
        st[1, 1] = np.nan
        st[2, 2] = 0.0            # division by a zero duration (unguarded in the reference too, onedpath_ip.cpp:385)
        b.set_state(st)
        b.solve(1e-8, 30, 0)
        it, status = b.get_iters()
        out = b.get_state()
        assert status[0] == rp.ST_CONVERGED and status[3] == rp.ST_CONVERGED
        assert np.array_equal(out[0], out[3])
        assert status[1] & rp.ST_NONFINITE and status[1] & rp.ST_MAXITER and it[1] == 30


def test_degenerate_problems_are_flagged_and_do_not_disturb_their_neighbours(oracle):
    # positions that make no problem (NaN, a zero-length segment: the start rule gives duration 0 and the first step divides by
    # it, unguarded in the reference too) among good ones, through the path a fresh batch takes: scheduling pass (their keys go
    # to the last ratio class), feasible start formed in registers, fused solve.  They end flagged; every other problem is
    # solved exactly as in a batch without them.
    n = 4096 + 77
    p0, p1, p2 = rp.problems.generate(606, 0, n, rp.problems.DIST_MONOTONE)
    q0, q1, q2 = p0.copy(), p1.copy(), p2.copy()
    bad = np.array([5, 64, 1000, 4096, n - 1])
    q1[bad[0]] = np.nan
    q1[bad[1]] = q0[bad[1]]                     # first segment empty
    q2[bad[2]] = q1[bad[2]]                     # second segment empty
    q0[bad[3]] = q1[bad[3]] = q2[bad[3]] = 7.0   # no trajectory at all
    q2[bad[4]] = np.inf
    good = np.ones(n, dtype=bool)
    good[bad] = False
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        a.solve(1e-8, 40, 0)
        b.set_problems(q0, q1, q2)
        b.solve(1e-8, 40, 0)
        ia, sa = a.get_iters()
        ib, sb = b.get_iters()
        xa, xb = a.get_state(), b.get_state()
    assert np.all(sa == rp.ST_CONVERGED)
    assert np.array_equal(ib[good], ia[good]) and np.array_equal(sb[good], sa[good]) and np.array_equal(xb[good], xa[good])
    assert not np.any(sb[bad] & rp.ST_CONVERGED)
    assert np.all((sb[bad] & (rp.ST_NONFINITE | rp.ST_MAXITER | rp.ST_INFEASIBLE)) != 0), sb[bad]


def test_nudges_match_special_keys():
    with rp.Batch(5) as b:
        b.init_default()
        b.nudge(1, 0.1); b.nudge(2, -0.1); b.nudge(0, 1.0); b.nudge(13, -10.0)
        st = b.get_state()
        assert np.allclose(st[:, 1], 3.6) and np.allclose(st[:, 2], 3.4) and np.all(st[:, 0] == 1.0) and np.all(st[:, 13] == 190.0)
        with pytest.raises(rp.RpError):
            b.nudge(16, 1.0)


def test_params_change_behaviour_and_are_validated(oracle):
    with rp.Batch(8) as b:
        with pytest.raises(rp.RpError):
            b.set_params(backtrack=1.5)
        b.set_params(accel_limit=50.0)
        assert b.get_params().accel_limit == 50.0
        b.set_problems(np.zeros(8), np.full(8, 100.0), np.full(8, 250.0))
        b.solve(1e-8, 200, 0)
        st = b.get_state()
        pos, acc = b.sample()
        assert np.max(np.abs(acc)) <= 50.0 * (1 + 1e-9)             # the tighter limit binds
        assert np.max(np.abs(acc)) > 49.99


# ---------------------------------------------------------------- reduction
def test_reduction_against_oracle(oracle, g3):
    n = 3000
    with rp.Batch(n) as b:
        b.set_state(g3["init"][:n])
        b.step(3)
        st = b.get_state()
        r = b.reduce()
    gaps = np.array([oracle.gap(3, row) for row in st])
    res = np.array([oracle.residual_norm(3, row, g / 80.0) for row, g in zip(st, gaps)])
    assert abs(r["max_gap"] / gaps.max() - 1) < 1e-12
    assert abs(r["max_residual_sq"] / res.max() - 1) < 1e-12
    assert r["n_converged"] == 0 and r["total_steps"] == 3.0 * n


# ---------------------------------------------------------------- F4
def test_f4_fp64_single_steps(golden_dir):
    t = np.load(os.path.join(golden_dir, "f4_steps.npz"))
    n = len(t["state_in"])
    with rp.Batch(n, variant=rp.VARIANT_F4, dtype=rp.DTYPE_F64) as b:
        b.set_state(t["state_in"])
        assert np.array_equal(b.get_state(), t["state_in"])
        b.step(1)
        st = b.get_state()
    assert serr(st[:, :3], t["state_out"][:, :3]) < TOL
    assert serr(st[:, 3:7], t["state_out"][:, 3:7]) < 1e-9


def test_f4_fp32_single_steps(golden_dir):
    # config 5: fp32; F4 trajectories are chaotic, so parity is per step from identical (fp32-exact) states
    t = np.load(os.path.join(golden_dir, "f4_steps.npz"))
    n = len(t["state_in"])
    with rp.Batch(n, variant=rp.VARIANT_F4, dtype=rp.DTYPE_F32) as b:
        b.set_state(t["state_in"])
        assert np.array_equal(b.get_state(), t["state_in"])          # inputs are fp32-representable
        b.step(1)
        st = b.get_state()
    err = np.abs(st[:, :3] - t["state_out"][:, :3]) / np.maximum(np.abs(t["state_out"][:, :3]), 1.0)
    assert np.all(np.isfinite(st))
    # fp32 tolerance: the step solves an ill-conditioned 3x3 system in single precision
    assert np.median(err) < 1e-5
    assert np.quantile(err, 0.99) < 2e-3


F32_ALIKE_TOL = 2.0e-3      # pure fp32 against fp32 state + fp64 arithmetic on problems whose line-search decisions agree: the direction's
                            # single-precision error, cond(K) x 6e-8 with cond(K) up to ~1e4 (profiles/r2_f4_fp32_error_tail.log), times s |dx| / |x| <= ~1
F32_STATE_TOL = 1.0e-7      # 2^-24 = 5.96e-8 (rounding of the result to fp32) + what fp64 arithmetic disagrees on (2.4e-11 measured)


def test_f4_fp32_state_single_steps_are_bounded_for_every_problem(golden_dir):
    # config 5 with a per-problem bound: fp32 state in HBM, fp64 arithmetic in registers.
    # One step from an fp32-representable state = the fp64 reference step, rounded to fp32 -- for EVERY problem.
    t = np.load(os.path.join(golden_dir, "f4_steps.npz"))
    n = len(t["state_in"])
    with rp.Batch(n, variant=rp.VARIANT_F4, dtype=rp.DTYPE_F32_STATE) as b:
        b.set_state(t["state_in"])
        assert np.array_equal(b.get_state(), t["state_in"])
        b.step(1)
        st = b.get_state()
    assert np.array_equal(st, st.astype(np.float32).astype(np.float64))      # the state is fp32
    err = np.abs(st[:, :3] - t["state_out"][:, :3]) / np.maximum(np.abs(t["state_out"][:, :3]), 1.0)
    assert err.max() < F32_STATE_TOL, err.max()
    assert lam_err(st[:, 3:7], t["state_out"][:, 3:7]) < F32_STATE_TOL
    assert np.array_equal(st[:, 7:], t["state_in"][:, 7:])


def test_fp32_state_fused_steps_equal_single_steps_bitwise(golden_dir):
    # the state is rounded to fp32 after every step whatever the launch shape
    t = np.load(os.path.join(golden_dir, "f4_steps.npz"))
    n = 2048
    with rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32_STATE) as a, rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32_STATE) as b:
        a.set_state(t["state_in"][:n])
        b.set_state(t["state_in"][:n])
        a.step(6)
        for _ in range(6):
            b.step(1)
        assert np.array_equal(a.get_state(), b.get_state())


def test_f3_fp32_state_gated_solve_reaches_the_fp64_optimum(oracle):
    # the same storage mode on F3: the solve converges to the fp64 optimum within fp32 resolution of the state
    n = 8192
    p0, p1, p2 = rp.problems.generate(55, 0, n, rp.problems.DIST_MONOTONE)
    p0, p1, p2 = (x.astype(np.float32).astype(np.float64) for x in (p0, p1, p2))
    aos = oracle.batch_init_feasible(3, p0, p1, p2)
    oracle.batch_solve_gated(3, aos, 1e-8, 200)
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F32_STATE) as b:
        b.set_problems(p0, p1, p2)
        b.solve(1e-3, 200, 0)                 # fp32 multipliers: a gap of 1e-8 is below what the state can hold
        st = b.get_state()
        _, status = b.get_iters()
    assert np.mean(status == rp.ST_CONVERGED) > 0.999
    assert serr(st[:, :3], aos[:, :3]) < 1e-3                # the gate: a surrogate gap of 1e-3 on a duration sum of ~5


def test_f4_default_trajectory(traj):
    with rp.Batch(1, variant=rp.VARIANT_F4) as b:
        b.init_default()
        for s in range(1, 9):
            b.step(1)
            assert serr(b.get_state()[0, :3], traj["f4_default_states"][s, :3]) < 1e-9, s


# ---------------------------------------------------------------- the rows either side of the path
def test_sample_against_oracle(oracle, g3):
    n = 500
    with rp.Batch(n) as b:
        b.set_state(g3["init"][:n])
        b.step(5)
        st = b.get_state()
        pos, acc = b.sample()
    for i in range(0, n, 7):
        p, a = oracle.sample(3, st[i])
        assert serr(pos[i], p) < 1e-13 and serr(acc[i], a) < 1e-13


def test_sample_into_device_memory_equals_the_host_read_back():
    from hip_util import DeviceBuffer
    n = 3 * 4096 + 17                                            # ragged last block of the kernel (128 problems per block)
    p0, p1, p2 = rp.problems.generate(606, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as b, DeviceBuffer(n * 66 * 8, fill=0xff) as d_pos, DeviceBuffer(n * 4 * 8, fill=0xff) as d_acc:
        b.set_problems(p0, p1, p2)
        b.solve(1e-8, 200, 0)
        pos, acc = b.sample()
        b.sample_device(d_pos.ptr, d_acc.ptr)
        # the device call takes a whole batch through problem-order records (k_solution + k_sample_records), the host call gathers
        # field by field (k_sample): same bits
        assert np.array_equal(d_pos.read(np.float64).reshape(n, 66), pos) and np.array_equal(d_acc.read(np.float64).reshape(n, 4), acc)
        # end points of the plot are the nodes themselves; the accelerations respect the limit at the solution
        st = b.get_state()
        assert np.array_equal(pos[:, 0], st[:, 11]) and np.array_equal(pos[:, 32], st[:, 13]) and np.array_equal(pos[:, 65], st[:, 14])
        assert np.abs(acc).max() <= 100.0 * (1 + 1e-12)
        # once a position has been moved the records are no longer the batch's positions: the device call must gather as well
        b.nudge(13, 10.0)                                        # Up key: pos1X += 10 for every problem
        pos2, acc2 = b.sample()
        b.sample_device(d_pos.ptr, d_acc.ptr)
        assert np.array_equal(d_pos.read(np.float64).reshape(n, 66), pos2) and np.array_equal(d_acc.read(np.float64).reshape(n, 4), acc2)
        assert np.array_equal(pos2[:, 32], pos[:, 32] + 10.0)
        # ... and after new problems it goes through the records again (F4, fp32 state: the records' positions are rounded as the fields are)
    with rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32_STATE) as b, DeviceBuffer(n * 66 * 8, fill=0xff) as d_pos, DeviceBuffer(n * 4 * 8, fill=0xff) as d_acc:
        b.set_problems(p0, p1, p2)
        b.step(7)
        pos, acc = b.sample()
        b.sample_device(d_pos.ptr, d_acc.ptr)
        assert np.array_equal(d_pos.read(np.float64).reshape(n, 66), pos) and np.array_equal(d_acc.read(np.float64).reshape(n, 4), acc)


def _violating_starts(oracle, variant, n, seed, four):
    """Feasible starts pushed out of the feasible set.  four=False: 1-3 violated accelerations (durations a little
    short and/or a large midpoint velocity).  four=True: both durations much too short, so that all four end
    accelerations exceed L -- four violated rows whose 4x4 Gram matrix has rank <= 3 (three variables): the
    rank-revealing branch of the QR (ColPivHouseholderQR.h:509, 524-525, 594-610)."""
    rng = np.random.RandomState(seed)
    p0, p1, p2 = rp.problems.generate(31 + seed, 0, n, 0)
    aos = oracle.batch_init_feasible(variant, p0, p1, p2)
    if four:
        aos[:, 1] *= rng.uniform(0.3, 0.8, n)
        aos[:, 2] *= rng.uniform(0.3, 0.8, n)
        aos[:, 0] = rng.uniform(-5, 5, n)
    else:
        aos[:, 1] *= rng.uniform(0.5, 1.2, n)
        aos[:, 2] *= rng.uniform(0.5, 1.2, n)
        aos[:, 0] = rng.uniform(-50, 250, n)
    m = oracle.num_constraints(variant)
    nviol = np.array([sum(oracle.constraint(variant, i, row)[0] > 0 for i in range(m)) for row in aos])
    return aos, nviol


@pytest.mark.parametrize("variant", [rp.VARIANT_F3, rp.VARIANT_F4])
@pytest.mark.parametrize("four", [False, True])
def test_move_toward_feasibility_against_oracle(oracle, variant, four):
    # moveTowardFeasibility, onedpath_ip.cpp:648-721 / onedpath2_ip.cpp:536-609.  The device code is an
    # operation-for-operation transcription (csrc/feas_core.h) in the order of Eigen's dynamic-size kernels, so the
    # comparison is bit for bit -- including the rank-deficient case (four violated rows, 3 variables), where the
    # reference's own answer hangs on the rounding of a pivot that is zero in exact arithmetic and no tolerance is
    # meaningful.  The oracle is pinned bit for bit on the reference's own function for 0-4 violated rows
    # (tests/test_oracle_reference.py); where the compiled reference travelled with the snapshot (oracle/_ref) the GPU
    # result is compared with it directly as well.
    n = 3000
    aos, nviol = _violating_starts(oracle, variant, n, 5 if four else 11, four)
    with rp.Batch(n, variant) as b:
        b.set_state(aos)
        b.move_toward_feasibility()
        out = b.get_state()
    exp = aos.copy()
    for row in exp:
        oracle.move_toward_feasibility(variant, row)
    if four:
        assert (nviol == 4).sum() > 2000
    else:
        assert ((nviol >= 1) & (nviol <= 3)).sum() > 800 and (nviol == 0).sum() > 100
    diff = np.any(out != exp, axis=1)
    err = np.max(np.abs(out[:, :3] - exp[:, :3]) / np.maximum(np.abs(exp[:, :3]), 1.0), axis=1)
    print("feasibility move variant %d four=%s: %d of %d rows differ from the oracle in any bit, max err %.2e" % (variant, four, diff.sum(), n, err.max()))
    assert np.array_equal(out, exp)
    import oracle_api
    if oracle_api.have_ref_hotpath():                                 # the reference's own moveTowardFeasibility
        assert np.array_equal(out, oracle_api.Reference().batch_move_toward_feasibility(variant, aos.copy()))
    assert np.array_equal(out[nviol == 0], aos[nviol == 0])           # nothing violated: no move
    assert np.array_equal(out[:, 3:], aos[:, 3:])                     # multipliers and constants untouched


@pytest.mark.parametrize("dtype", [rp.DTYPE_F32, rp.DTYPE_F32_STATE])
def test_move_toward_feasibility_from_fp32_states(oracle, dtype):
    # The move is computed in double whatever the batch's arithmetic type (it squares the conditioning of the gradients:
    # in single precision 10 % of the moves were off by more than 6e-3), so an fp32 state gets the reference's move
    # rounded to fp32 -- a per-problem bound.
    n = 2000
    aos, _ = _violating_starts(oracle, rp.VARIANT_F4, n, 3, four=False)
    aos = aos.astype(np.float32).astype(np.float64)
    nviol = np.array([sum(oracle.constraint(4, i, row)[0] > 0 for i in range(4)) for row in aos])
    with rp.Batch(n, rp.VARIANT_F4, dtype) as b:
        b.set_state(aos)
        b.move_toward_feasibility()
        out = b.get_state()
    exp = aos.copy()
    for row in exp:
        oracle.move_toward_feasibility(4, row)
    ok = (nviol >= 1) & (nviol <= 3)
    assert ok.sum() > 800
    err = np.max(np.abs(out[ok, :3] - exp[ok, :3]) / np.maximum(np.abs(exp[ok, :3]), 1.0), axis=1)
    assert err.max() < 1.0e-7
    assert np.array_equal(out[nviol == 0], aos[nviol == 0])


# ---------------------------------------------------------------- the C++ plug-in through the headless shell
def test_headless_shell_reproduces_the_survey_kats(golden_dir):
    import json
    exe = os.path.join(ROOT, "rocket_path_amd", "lib", "rp_headless")
    kat = json.load(open(os.path.join(golden_dir, "survey_kat.json")))["f3_default"]
    out = subprocess.run([exe, "--n", "1", "--keys", "i n s n s n13 s"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    states = [list(map(float, l.split()[1:])) for l in out.stdout.splitlines() if l.startswith("State17:")]
    assert len(states) == 3
    assert serr(states[0], kat["after_step_1"]) < 1e-11
    assert serr(states[1], kat["after_step_2"]) < 1e-11
    assert serr(states[2][:3], kat["after_step_15_v_t0_t1"]) < 1e-12
    assert "Node 1: pos=200" in out.stdout and "Duration 0:" in out.stdout


# ---------------------------------------------------------------- the fused gated solve on large batches
def test_fused_solve_ragged_tail_and_resume(oracle):
    # 4,101 full 64-problem chunks of the scheduled order + a 13-problem tail
    n = 512 * 512 + 333
    p0, p1, p2 = rp.problems.generate(4242, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        a.solve(1e-8, 200, 0)            # fused: one launch
        b.solve(1e-8, 200, 7)            # the same kernel in host-polled rounds of 7 steps
        sa, sb = a.get_state(), b.get_state()
        ia, ta = a.get_iters()
        ib, tb = b.get_iters()
        assert np.array_equal(sa, sb) and np.array_equal(ia, ib) and np.array_equal(ta, tb)   # the launch shape changes nothing
        assert a.reduce()["total_steps"] == float(ia.sum())
        # resume: a capped solve continued later equals the uninterrupted one
        b.set_problems(p0, p1, p2)
        b.solve(1e-8, 9, 0)
        i9, t9 = b.get_iters()
        assert np.all(i9 == 9) and np.all(t9 & rp.ST_MAXITER)
    for sl in (slice(0, 4096), slice(n - 4096, n)):
        init = oracle.batch_init_feasible(3, p0[sl], p1[sl], p2[sl])
        aos = init.copy()
        it_o, _ = oracle.batch_solve_gated(3, aos, 1e-8, 200)
        ok = keep_mask(len(it_o), certify_iteration_counts(oracle, 3, init, ia[sl], it_o, 1e-8))
        assert serr(sa[sl, :3][ok], aos[ok, :3]) < TOL


def test_fused_solve_survives_a_stale_order():
    # nudging positions after the scheduled order was computed only makes the schedule less effective: same results as a
    # batch that was scheduled on the nudged positions
    n = 512 * 512
    p0, p1, p2 = rp.problems.generate(99, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        a.nudge(13, 10.0)                 # Up key: pos1 += 10 for every problem, order now stale
        st = a.get_state()
        b.set_state(st)                   # same state, fresh order
        a.solve(1e-8, 200, 0)
        b.solve(1e-8, 200, 0)
        assert np.array_equal(a.get_state(), b.get_state())
        assert np.array_equal(a.get_iters()[0], b.get_iters()[0])


def test_fused_solve_f4_fp32_matches_the_host_polled_rounds():
    n = 512 * 512 + 5
    p0, p1, p2 = rp.problems.generate(5, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32) as a, rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        a.solve(1e-3, 25, 0)
        b.solve(1e-3, 25, 5)
        assert np.array_equal(a.get_state(), b.get_state())
        assert np.array_equal(a.get_iters()[0], b.get_iters()[0])


# ---------------------------------------------------------------- stall detector, off by default
def test_stall_detector_is_off_by_default_and_stops_the_stuck_state(g3):
    n = 1024
    with rp.Batch(n) as b:
        assert b.get_params().stall_window == 0
        b.init_stuck()                        # initStuck, onedpath_ip.cpp:177-199: the gap stays ~2.08 for ever
        b.solve(1e-8, 60, 0)
        it, st = b.get_iters()
        assert np.all(it == 60) and np.all(st & rp.ST_MAXITER) and not np.any(st & rp.ST_STALLED)
        b.set_params(stall_window=8)
        b.init_stuck()
        b.solve(1e-8, 200, 0)
        it, st = b.get_iters()
        assert np.all(st & rp.ST_STALLED) and np.all(it < 40) and not np.any(st & rp.ST_CONVERGED)
        stuck = b.get_state()
        b.solve(1e-8, 200, 0)                 # a stalled problem is left alone
        assert np.array_equal(b.get_state(), stuck)
        # a converging batch is untouched by the detector: bit-identical to the golden run without it
        b.set_state(g3["init"][:n])
        b.solve(1e-8, 200, 0)
        it, st = b.get_iters()
        assert np.array_equal(it, g3["iters"][:n]) and np.all(st == rp.ST_CONVERGED)
        assert serr(b.get_state()[:, :3], g3["gated"][:n, :3]) < TOL


def test_sharded_cpp_host_with_rccl_on_one_device():
    # the single-process multi-GPU host class (csrc/host/sharded_problem.cpp) on the one device this box has:
    # shard bookkeeping, ncclCommInitAll, the grouped MAX/SUM all-reduce of the device-resident summary
    exe = os.path.join(ROOT, "rocket_path_amd", "lib", "rp_headless")
    n = 4096
    out = subprocess.run([exe, "--gpus", "1", "--n", str(n), "--seed", "12345", "--solve", "--keys", "s"],
                         capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("Batch:")][-1]
    p0, p1, p2 = rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as b:
        b.set_problems(p0, p1, p2)
        b.solve(1e-8, 200, 0)
        r = b.reduce()
    assert "converged: %d" % n in line and "steps: %.0f" % r["total_steps"] in line
    assert ("max surrogate gap: %g" % r["max_gap"]) in line
    # asking for more devices than exist is refused, not faked
    bad = subprocess.run([exe, "--gpus", "64", "--n", "128", "--keys", "s"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "visible" in bad.stderr


def test_zero_end_velocity_specialisation_is_bit_identical_to_the_general_kernels():
    # Every init the reference has leaves vel0X = vel2X = 0, and the kernels are instantiated for that case
    # (two fields not read, four multiply-adds fewer per evaluation).  A +1/-1 nudge of vel0X leaves the values at
    # zero but clears the batch's flag, i.e. selects the general instantiation: results must not differ by a bit.
    n = 512 * 512 + 100
    p0, p1, p2 = rp.problems.generate(321, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        b.nudge(12, 1.0); b.nudge(12, -1.0)           # vel0X (index 12 of enum V)
        assert np.array_equal(a.get_state(), b.get_state())
        a.step(3); b.step(3)                           # streaming kernel
        assert np.array_equal(a.get_state(), b.get_state())
        a.solve(1e-8, 200, 0); b.solve(1e-8, 200, 0)   # fused gated solve (k_solve_chunks)
        assert np.array_equal(a.get_state(), b.get_state()) and np.array_equal(a.get_iters()[0], b.get_iters()[0])
        a.set_problems(p0, p1, p2); b.set_problems(p0, p1, p2)
        b.nudge(15, 2.0); b.nudge(15, -2.0)            # vel2X
        a.solve(1e-8, 200, 3); b.solve(1e-8, 200, 3)   # the same kernel in rounds of 3 steps, host-polled
        assert np.array_equal(a.get_state(), b.get_state())


def test_non_zero_end_velocities_against_oracle(oracle, g3):
    m = 4096
    st = g3["init"][:m].copy()
    st[:, 12] = np.linspace(-3.0, 3.0, m)
    st[:, 15] = np.linspace(2.0, -2.0, m)
    exp = st.copy()
    oracle.batch_steps(3, exp, 4)
    with rp.Batch(m) as c:
        c.set_state(st)
        c.step(4)
        out = c.get_state()
    assert serr(out[:, :3], exp[:, :3]) < TOL
    assert np.array_equal(out[:, 11:], st[:, 11:])


def test_non_zero_end_velocities_through_the_large_batch_kernels_against_oracle(oracle):
    # the large-batch kernels' ZV=false instantiations (gated k_solve_chunks, ungated k_steps_chunks) had only
    # ever seen zero end velocities.
    # 512 full tiles + a ragged tail; end velocities small enough that the start stays feasible (|da| <= 0.4 of the
    # 2.04 margin of the feasible-start rule).
    n = 512 * 512 + 301
    p0, p1, p2 = rp.problems.generate(606, 0, n, rp.problems.DIST_MONOTONE)
    rng = np.random.RandomState(9)
    sl_list = (slice(0, 3000), slice(130000, 133000), slice(n - 3000, n))
    init = np.zeros((n, 16))
    for sl in (slice(0, n // 2), slice(n // 2, n)):
        init[sl] = oracle.batch_init_feasible(3, p0[sl], p1[sl], p2[sl])
    init[:, 12] = 0.1 * rng.uniform(-1, 1, n) * init[:, 1]
    init[:, 15] = 0.1 * rng.uniform(-1, 1, n) * init[:, 2]
    with rp.Batch(n) as b:
        b.set_state(init)
        b.solve(1e-8, 200, 0)                 # fused gated solve, general instantiation
        it, status = b.get_iters()
        st = b.get_state()
        b.set_state(init)
        b.step(5)                             # large-batch fixed steps (k_steps_chunks), general instantiation
        st5 = b.get_state()
    assert np.all(status == rp.ST_CONVERGED)
    assert np.array_equal(st[:, 11:], init[:, 11:])
    for sl in sl_list:
        exp = init[sl].copy()
        it_o, _ = oracle.batch_solve_gated(3, exp, 1e-8, 200)
        ok = keep_mask(len(it_o), certify_iteration_counts(oracle, 3, init[sl], it[sl], it_o, 1e-8))
        assert serr(st[sl, :3][ok], exp[ok, :3]) < TOL
        assert lam_err(st[sl, 3:11][ok], exp[ok, 3:11]) < LAM_TOL
        exp5 = init[sl].copy()
        oracle.batch_steps(3, exp5, 5)
        assert serr(st5[sl, :3], exp5[:, :3]) < TOL
    # and the velocities matter (the zero-end-velocity kernels would not have produced this)
    zero = init[sl_list[0]].copy()
    zero[:, 12] = 0.0
    zero[:, 15] = 0.0
    oracle.batch_steps(3, zero, 5)
    assert serr(st5[sl_list[0], :3], zero[:, :3]) > 1e-6


def test_large_batch_fixed_steps_equal_streamed_single_steps_bitwise():
    # k >= 3 on a large batch runs k_steps_chunks, k = 1 the streaming kernel: same arithmetic, same bits
    n = 512 * 512 + 77
    p0, p1, p2 = rp.problems.generate(2025, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        a.step(5)
        for _ in range(5):
            b.step(1)
        assert np.array_equal(a.get_state(), b.get_state())
        it, _ = a.get_iters()
        assert np.all(it == 5)


@pytest.mark.parametrize("variant,dtype", [(rp.VARIANT_F3, rp.DTYPE_F64), (rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F4, rp.DTYPE_F32_STATE)])
@pytest.mark.parametrize("n", [4096 + 17, 512 * 512 + 33])
def test_launch_shapes_agree_through_the_post_convergence_regime(variant, dtype, n):
    # 50 steps of the default problem run ~30 of them in the reference's post-convergence regime (x no longer moves, ~48
    # residual halvings per step).  One launch of 50, launches of 2 + 16 + 32 (chunk kernel) and 50 single-step launches
    # (streaming kernel), plus the diagnostic kernel: every fixed-step kernel of a variant walks the same arithmetic in that
    # regime (F4: affine residual pieces; F3: the direct evaluation -- kAffine in ip_kernels.hip), so they agree bit for bit,
    # multipliers included.
    with rp.Batch(n, variant, dtype) as a, rp.Batch(n, variant, dtype) as b, rp.Batch(n, variant, dtype) as c, rp.Batch(n, variant, dtype) as d:
        for x in (a, b, c, d):
            x.init_default()
        a.step(50)
        for k in (2, 16, 32):
            b.step(k)
        for _ in range(50):
            c.step(1)
        d.step_counted(50)
        sa, sb, sc, sd = a.get_state(), b.get_state(), c.get_state(), d.get_state()
    assert np.all(sa == sa[0])                                # identical problems, identical results in every lane
    assert np.array_equal(sa, sb) and np.array_equal(sa, sc) and np.array_equal(sa, sd)


def test_f4_fused_steps_with_another_backtrack_factor_equal_single_steps_bitwise():
    # the wave-parallel service needs the reference's backtrack factor 1/2 (its step lengths s 2^-q are exact); with any other
    # factor the fused kernel keeps to the wave-uniform lock-step loop, which must still be the serial loop bit for bit
    n = 4096 * 3 + 5
    p0, p1, p2 = rp.problems.generate(31337, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F64) as a, rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F64) as b:
        for x in (a, b):
            x.set_params(backtrack=0.25, max_backtracks=40)
            x.set_problems(p0, p1, p2)
        a.step(24)
        for _ in range(24):
            b.step(1)
        sa, sb = a.get_state(), b.get_state()
        assert np.all(np.isfinite(sa)) and np.array_equal(sa, sb)


# ---------------------------------------------------------------- mu schedule option, F4 settling flag
def test_mu_mode_defaults_to_the_reference_and_is_validated(g3):
    n = 2048
    with rp.Batch(n) as b:
        p = b.get_params()
        assert p.mu_mode == 0 and (p.mu_sigma_try[0], p.mu_sigma_try[1]) == (0.01, 0.03)
        with pytest.raises(rp.RpError):
            b.set_params(mu_mode=2)
        b.set_params(mu_mode=1)
        b.set_state(g3["init"][:n])
        b.solve(1e-8, 200, 0)
        b.set_params(mu_mode=0)              # back to the reference: bit-identical to the golden run
        b.set_state(g3["init"][:n])
        b.solve(1e-8, 200, 0)
        it, status = b.get_iters()
        assert np.array_equal(it, g3["iters"][:n]) and serr(b.get_state()[:, :3], g3["gated"][:n, :3]) < TOL
    with rp.Batch(8, rp.VARIANT_F4, rp.DTYPE_F32) as c:
        with pytest.raises(rp.RpError):
            c.set_params(mu_mode=1)          # centring by trial needs double arithmetic


@pytest.mark.parametrize("steps_per_launch", [0, 6])
def test_mu_mode_1_reaches_the_same_optimum_in_fewer_steps(steps_per_launch):
    n = 20000
    p0, p1, p2 = rp.problems.generate(2468, 0, n, rp.problems.DIST_MONOTONE)      # the C3 distribution
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        b.set_params(mu_mode=1)
        a.solve(1e-8, 200, steps_per_launch)
        b.solve(1e-8, 200, steps_per_launch)
        ia, sa = a.get_iters()
        ib, sb = b.get_iters()
        xa, xb = a.get_state(), b.get_state()
        gb = b.reduce()["max_gap"]
    assert np.all(sa == rp.ST_CONVERGED) and np.all(sb == rp.ST_CONVERGED) and gb < 1e-8
    print("mean steps: reference %.2f, centring by trial %.2f (max %d / %d)" % (ia.mean(), ib.mean(), ia.max(), ib.max()))
    assert ib.mean() < 0.9 * ia.mean() and ib.max() <= ia.max()
    assert serr(xb[:, :3], xa[:, :3]) < 1e-8          # both stop at a gap below 1e-8: same optimum to that accuracy


def test_mu_mode_1_ungated_steps_and_the_stuck_state():
    n = 4096
    p0, p1, p2 = rp.problems.generate(97, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        b.set_params(mu_mode=1)
        a.step(10)
        b.step(10)
        _, acc = b.sample()
        assert np.all(np.isfinite(b.get_state())) and np.max(np.abs(acc)) <= 100.0      # the trial steps keep feasibility too
        a.solve(1e-8, 200, 0)
        b.solve(1e-8, 200, 0)                    # ungated steps and the gated solve mix freely
        assert np.all(b.get_iters()[1] == rp.ST_CONVERGED) and b.get_iters()[0].mean() < a.get_iters()[0].mean()
        assert serr(b.get_state()[:, :3], a.get_state()[:, :3]) < 1e-8
        # initStuck (onedpath_ip.cpp:177-199): converges or is flagged, never spins silently
        b.set_params(mu_mode=1, stall_window=8)
        b.init_stuck()
        b.solve(1e-8, 200, 0)
        it, st = b.get_iters()
        assert np.all((st & rp.ST_CONVERGED) | (st & rp.ST_STALLED)) and np.all(it < 200)


def test_f4_wrong_way_settling_is_flagged_with_the_stall_detector_on():
    # F4 never converges from the feasible start: its duration sum grows while the gap sticks (README.md:34)
    n = 1024
    p0, p1, p2 = rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n, rp.VARIANT_F4) as b:
        b.set_problems(p0, p1, p2)
        t_in = b.get_state()[:, 1:3].sum(axis=1)
        b.solve(1e-6, 60, 0)
        _, st = b.get_iters()
        assert not np.any(st & rp.ST_WRONG_WAY) and np.all(st & rp.ST_MAXITER)      # detector off: the reference's behaviour
        b.set_params(stall_window=8)
        b.set_problems(p0, p1, p2)
        b.solve(1e-6, 200, 0)
        it, st = b.get_iters()
        t_out = b.get_state()[:, 1:3].sum(axis=1)
    assert np.all(st & rp.ST_STALLED) and not np.any(st & rp.ST_CONVERGED) and np.all(it < 60)
    wrong = (st & rp.ST_WRONG_WAY) != 0
    assert np.array_equal(wrong, ~(t_out < t_in)) and wrong.mean() > 0.5
    with rp.Batch(n) as c:                                     # F3 on the same problems converges and is never flagged
        c.set_params(stall_window=8)
        c.set_problems(p0, p1, p2)
        c.solve(1e-8, 200, 0)
        _, st3 = c.get_iters()
    assert np.all(st3 == rp.ST_CONVERGED)


@pytest.mark.parametrize("steps_per_launch", [1, 4])
def test_wrong_way_flag_does_not_outlive_convergence_in_short_launches(steps_per_launch):
    # RP_ST_WRONG_WAY is decided per launch (objective at the launch's start).  In host-polled rounds of 1 or 4 steps an F3
    # problem's duration sum does not drop in every round (the first steps of a solve raise it: 3.5 -> 3.67 on the default
    # problem), so the flag is raised on the way -- and must be gone once the problem has converged.
    n = 4096
    p0, p1, p2 = rp.problems.generate(515, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n) as b, rp.Batch(n) as ref:
        b.set_params(stall_window=8)
        b.set_problems(p0, p1, p2)
        b.solve(1e-8, 200, steps_per_launch)
        it, st = b.get_iters()
        ref.set_problems(p0, p1, p2)
        ref.solve(1e-8, 200, 0)
        it_ref, st_ref = ref.get_iters()
        assert np.all(st == rp.ST_CONVERGED) and np.all(st_ref == rp.ST_CONVERGED)
        assert np.array_equal(it, it_ref) and np.array_equal(b.get_state(), ref.get_state())


# ---------------------------------------------------------------- decision-level parity of the line search
def test_halving_counts_equal_the_oracles_step_by_step(oracle):
    # rp_batch_step_counted = rp_batch_step + how often each of the two backtracking loops halved the step
    # (onedpath_ip.cpp:927, 944): the same counts as the oracle's orc_step_info, problem by problem, step by step,
    # for as long as the iteration is above rounding level (gap >= ~1e-11: the first 16 steps of this distribution;
    # from ~step 19 on both sides take their decisions on the last bit of |a| - L and on whether lam + s dlam still
    # rounds to lam, and the counts are noise on both -- profiles/r2_halving_probe.log).
    n = 2048
    p0, p1, p2 = rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)
    aos = oracle.batch_init_feasible(3, p0, p1, p2)
    info = StepInfo()
    with rp.Batch(n) as a, rp.Batch(n) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        tot_f = tot_r = 0
        for s in range(16):
            nf, nr = a.step_counted(1)
            b.step(1)
            of = np.zeros(n, dtype=np.uint32)
            orr = np.zeros(n, dtype=np.uint32)
            for i in range(n):
                oracle.step(3, aos[i], info)
                of[i], orr[i] = info.feas_halvings, info.resid_halvings
            assert np.array_equal(nf, of) and np.array_equal(nr, orr), s
            tot_f += int(of.sum())
            tot_r += int(orr.sum())
        assert tot_f > 3000                                   # the comparison is not vacuous: ~0.2 halvings per step
        assert np.array_equal(a.get_state(), b.get_state())   # the counted twin computes the very same steps
        assert np.array_equal(a.get_iters()[0], b.get_iters()[0])
        # ... and keeps doing so through the post-convergence regime (memoised trial points, affine residual pieces, the
        # closed-form tail of a feasibility loop stuck on x vs. its counted loop form): 30 more steps, still bit for bit
        for s in range(30):
            nf, nr = a.step_counted(1)
            b.step(1)
        assert nr.max() >= 40 and nf.max() == 100             # the regime was reached: ~50 residual halvings, stuck feasibility loops
        assert np.array_equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("variant,dist,steps", [(rp.VARIANT_F3, rp.problems.DIST_NON_MONOTONE, 12), (rp.VARIANT_F3, rp.problems.DIST_REFERENCE_LIKE, 14),
                                                (rp.VARIANT_F4, rp.problems.DIST_MONOTONE, 10)])
def test_halving_counts_on_the_other_distributions_and_f4(oracle, variant, dist, steps):
    # the same decision-level comparison on the stress / reference-like sets and on F4 (whose line search is the busy one:
    # several feasibility halvings per step from step ~4 on)
    n = 1024
    p0, p1, p2 = rp.problems.generate(4711, 0, n, dist)
    aos = oracle.batch_init_feasible(variant, p0, p1, p2)
    info = StepInfo()
    mism = total = 0
    with rp.Batch(n, variant) as a:
        a.set_problems(p0, p1, p2)
        for s in range(steps):
            nf, nr = a.step_counted(1)
            for i in range(n):
                oracle.step(variant, aos[i], info)
                mism += int(nf[i] != info.feas_halvings) + int(nr[i] != info.resid_halvings)
                total += info.feas_halvings + info.resid_halvings
        st = a.get_state()
    assert total > 200
    assert mism == 0, "%d of %d decisions differ" % (mism, 2 * n * steps)
    # F4 trajectories are chaotic (rounding-level differences grow ~10x every few steps; parity of its states
    # is pinned per step from identical states, test_f4_fp64_single_steps): after 10 steps only the decisions are compared tightly
    assert serr(st[:, :3], aos[:, :3]) < (TOL if variant == rp.VARIANT_F3 else 1e-5)


def test_f4_halving_counts_in_the_long_sequence_regime(oracle):
    # From step ~10 on F4 halves the step 12-19 times at every other step of a problem.  The device walks those sequences
    # without evaluating their trials: the number of halvings that are infeasible beyond doubt comes from a closed form along
    # the ray (ip_core.h: ray_proof, bisection over the count), the next few from a division-free per-trial proof
    # (infeasible_beyond_doubt), the last one or two from the evaluation proper.  One step from states the ORACLE reached after
    # 24 steps: both halving counts of every problem against the oracle's.
    n = 2048
    p0, p1, p2 = rp.problems.generate(2718, 0, n, rp.problems.DIST_MONOTONE)
    aos = oracle.batch_init_feasible(rp.VARIANT_F4, p0, p1, p2)
    oracle.batch_steps(rp.VARIANT_F4, aos, 24)
    info = StepInfo()
    before = aos.copy()
    with rp.Batch(n, rp.VARIANT_F4) as a:
        a.set_state(aos)
        nf, nr = a.step_counted(1)
        got = a.get_state()
    exp_nf, exp_nr = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        oracle.step(rp.VARIANT_F4, aos[i], info)
        exp_nf[i], exp_nr[i] = info.feas_halvings, info.resid_halvings
    long_ones = exp_nf >= 10
    assert long_ones.sum() > n // 4 and exp_nf.max() >= 17            # the regime was reached
    assert np.array_equal(nf, exp_nf), "%d feasibility counts differ" % int((nf != exp_nf).sum())
    # the residual loop of a stalled F4 problem ends where s dr drops below the rounding of |r|^2 (~50 halvings): that last-bit
    # decision differs between the condensed 3 x 3 solve and the reference's QR on a few problems per thousand (6 of 2,048
    # measured), as in F3's post-convergence regime (profiles/r2_halving_probe.log); the feasibility counts above do not.  Each
    # such difference is CERTIFIED (parity_util.certify_line_search_decisions): at the first trial the two sides decide differently
    # the oracle's own |r(trial)|^2 lies within rounding of its threshold (RESID_TIE one-ulp spreads) -- any other difference fails here
    cert = certify_line_search_decisions(oracle, rp.VARIANT_F4, before, nf, nr, exp_nf, exp_nr)
    print("F4 long-sequence regime: %d of %d residual counts differ, all certified ties (worst %.2f of the allowance)"
          % (cert["resid_diffs"], n, cert["worst_resid"]))
    same = nr == exp_nr
    assert serr(got[same, :3], aos[same, :3]) < 1e-9


@pytest.mark.parametrize("dtype", [rp.DTYPE_F64, rp.DTYPE_F32_STATE, rp.DTYPE_F32])
def test_f4_wave_parallel_line_search_equals_single_steps_bitwise(dtype):
    # F4's fused fixed-step launches serve the stragglers of the residual loop with the whole wave (newton_step_to, WAVE:
    # the straggler's state is broadcast, every live lane evaluates one of its next 64 step lengths, a ballot finds the first
    # trial the serial loop would stop at).  The single-step launches run the serial loop.  Which lane evaluated a trial must
    # not change a bit of any result -- through the regime where F4's problems walk ~50 residual halvings per step (from
    # step ~6 on for a growing share of them: this is what the service is for), with a ragged last wave (n % 64 = 13), and
    # the halving counts must be the serial loop's.
    n = 512 * 512 + 77
    p0, p1, p2 = rp.problems.generate(2026, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n, rp.VARIANT_F4, dtype) as a, rp.Batch(n, rp.VARIANT_F4, dtype) as b:
        a.set_problems(p0, p1, p2)
        b.set_problems(p0, p1, p2)
        a.step(14)                       # k_steps_chunks with the wave-parallel search
        for _ in range(14):
            b.step(1)                    # streaming kernel, serial search
        sa, sb = a.get_state(), b.get_state()
        assert np.all(np.isfinite(sa))
        assert np.array_equal(sa, sb)
        a.step(22)
        for _ in range(21):
            b.step(1)
        nf, nr = b.step_counted(1)       # the diagnostic kernel: serial too; by now the long residual loops are there
        assert np.array_equal(a.get_state(), b.get_state())
        assert np.all(a.get_iters()[0] == 36)
        assert (nr > 20).sum() > 30, (nr > 20).sum()      # ... so the service did run on the other side (fp64: ~1 % of the problems, fp32: a few dozen)


def _unpredicted_states(oracle, n, seed, family):
    """States whose step counts the batch's internal order says nothing about (what nudges, set_state and
    restored starts feed in): a few problems in each need several times the typical count, some the whole budget."""
    rng = np.random.default_rng(seed)
    p0, p1, p2 = rp.problems.generate(seed, 0, n, rp.problems.DIST_NON_MONOTONE if family == "durations" else rp.problems.DIST_MONOTONE)
    st = oracle.batch_init_feasible(3, p0, p1, p2)
    if family == "multipliers":
        st[:, 3:11] = 10.0 ** rng.uniform(-3, 2, (n, 1))
    elif family == "vel1":
        st[:, 0] = rng.uniform(-10, 10, n)
    elif family == "durations":
        st[:, 1] += rng.choice([0.0, 0.1, 1.0], n)
        st[:, 2] += rng.choice([0.0, 0.1, 1.0], n)
    return st


@pytest.mark.parametrize("family", ["multipliers", "vel1", "durations"])
def test_gated_solve_in_rounds_gives_every_problem_the_steps_of_the_single_launch(oracle, family):
    # states entered through set_state (multipliers != 1, a nudged velocity, nudged durations) have step counts the
    # scheduled order does not predict -- a few problems need 60 or 200 steps and hold their wave's other 63 lanes.  On request the fused
    # solve runs in rounds (rp_params.handoff_rounds = 2..8; 0, the default, watches for fixed points in one launch after a set_state):
    # waves hand their last stragglers off, later launches pack them densely.
    # Which lane runs a problem changes nothing: states, multipliers, iteration counts, status words and the bound
    # solution records must be bit for bit those of ONE launch (handoff_rounds = -1), for every round count, a small lane threshold,
    # a step budget that ends mid-solve, and a resumed solve.  The oracle checks the answers themselves.
    from hip_util import DeviceBuffer
    n = 48 * 1024 + 21
    st0 = _unpredicted_states(oracle, n, 4711, family)
    dt = np.dtype(rp.capi.SOLUTION_FIELDS)
    ref = {}
    with rp.Batch(n) as one, DeviceBuffer(32 * n) as out:
        one.set_params(handoff_rounds=-1)
        one.bind_solution(out.ptr)
        for cap in (200, 9):
            one.set_state(st0)
            one.solve(1e-8, cap, 0)
            ref[cap] = (one.get_state(), one.get_iters(), out.read(dt).copy(), one.reduce())
        one.solve(1e-8, 200, 0)                      # ... and the resumed solve from the 9-step state
        ref["resumed"] = (one.get_state(), one.get_iters(), out.read(dt).copy(), one.reduce())
    it200 = ref[200][1][0]
    assert it200.max() >= 3 * np.median(it200), (it200.max(), np.median(it200))      # the family really has stragglers
    for rounds, lanes in ((0, 24), (2, 24), (5, 8), (8, 48), (3, 1)):
        with rp.Batch(n) as b, DeviceBuffer(32 * n, fill=0xff) as out:
            b.set_params(handoff_rounds=rounds, handoff_lanes=lanes)
            b.bind_solution(out.ptr)
            for cap in (200, 9):
                b.set_state(st0)
                b.solve(1e-8, cap, 0)
                st, (it, status), rec, red = b.get_state(), b.get_iters(), out.read(dt), b.reduce()
                assert np.array_equal(st.view(np.uint64), ref[cap][0].view(np.uint64)), (rounds, lanes, cap, int((st.view(np.uint64) != ref[cap][0].view(np.uint64)).any(axis=1).sum()))
                assert np.array_equal(it, ref[cap][1][0]) and np.array_equal(status, ref[cap][1][1]), (rounds, lanes, cap)
                assert np.array_equal(rec.view(np.uint8), ref[cap][2].view(np.uint8)) and repr(red) == repr(ref[cap][3]), (rounds, lanes, cap)
            b.solve(1e-8, 200, 0)
            st, (it, status), rec, red = b.get_state(), b.get_iters(), out.read(dt), b.reduce()
            assert np.array_equal(st.view(np.uint64), ref["resumed"][0].view(np.uint64)) and np.array_equal(it, ref["resumed"][1][0]) and np.array_equal(status, ref["resumed"][1][1])
            assert np.array_equal(rec.view(np.uint8), ref["resumed"][2].view(np.uint8)) and repr(red) == repr(ref["resumed"][3])
    # the answers themselves: iteration counts and (v, t0, t1) against the oracle
    aos = st0.copy()
    it_o = np.asarray(oracle.batch_solve_gated(3, aos, 1e-8, 200)[0])
    # ... for the starts INSIDE the feasible set.  (A start outside it is outside the parity statement: the reference makes no progress from
    # one, 100 halvings and a frozen state -- test_infeasible_start_is_frozen_and_flagged -- unless its singular KKT system happens to
    # yield a direction of ~1e30, which a step length of 2^-100 turns into a real move: noise that no two solvers share.  A start ON a
    # limit is a tie of the first feasibility test.)  |a| <= L (1 - 1e-9) at all four ends, from the spline formulas of SURVEY 8a:
    v1, t0, t1, x0, x1, x2 = st0[:, 0], st0[:, 1], st0[:, 2], st0[:, 11], st0[:, 13], st0[:, 14]
    acc = np.stack([(6 * (x1 - x0) / t0 - 2 * v1) / t0, (-6 * (x1 - x0) / t0 + 4 * v1) / t0,
                    (6 * (x2 - x1) / t1 - 4 * v1) / t1, (-6 * (x2 - x1) / t1 + 2 * v1) / t1], axis=1)
    keep = np.max(np.abs(acc), axis=1) <= 100.0 * (1 - 1e-9)
    keep &= it_o <= 80      # (and for the problems that do not STALL: a stalled trajectory -- dozens of halvings per step for a hundred steps -- is noise-driven)
    assert keep.sum() > n // 2
    ok = keep_mask(keep.sum(), certify_iteration_counts(oracle, 3, st0[keep], it200[keep], it_o[keep], 1e-8, max_ties=16))
    done = ok & (it_o[keep] < 200)
    assert serr(ref[200][0][keep][done, :3], aos[keep][done, :3]) < 1e-9


def test_idle_lane_steps_of_states_entered_through_set_state(oracle):
    # VERDICT r5 next 4, the measurement it asks for first: batches entered through rp_batch_set_state with the nudges the reference's keys
    # make (durations +0.1 / +1, onedpath_ip.cpp:280-324), multipliers other than 1, and the three position distributions mixed and
    # shuffled.  A wave holds 64 consecutive positions of the batch's internal order and runs until its slowest lane is done: idle
    # lane-steps = 1 - sum(steps) / (64 * sum over waves of the wave's largest count), from the device's own iteration counts and slot map.
    # The position-derived order keeps it at or below 3 % for every one of them (1.0-2.3 % at 1 Mi problems, profiles/r6_state_families.log);
    # what it cannot know is a state whose step counts are heavy-tailed (a start outside the feasible set, per-problem multipliers over
    # five decades): those are the business of rp_params.handoff_rounds (tests above), not of the order.
    n = 256 * 1024
    rng = np.random.default_rng(2)
    base = oracle.batch_init_feasible(3, *rp.problems.generate(8675309, 0, n, rp.problems.DIST_MONOTONE))
    fams = {"feasible start": base}
    for d in (0.1, 1.0):
        x = base.copy(); x[:, 1] += d; x[:, 2] += d; fams["durations +%g" % d] = x
    for lam in (100.0, 0.01):
        x = base.copy(); x[:, 3:11] = lam; fams["multipliers %g" % lam] = x
    parts = [oracle.batch_init_feasible(3, *rp.problems.generate(77 + d, 0, n // 2 if d == 0 else n // 4, d)) for d in (0, 1, 2)]
    fams["three distributions mixed"] = np.concatenate(parts)[rng.permutation(n)]
    report = []
    with rp.Batch(n) as b:
        for name, st in fams.items():
            b.set_state(st)
            b.solve(1e-8, 200, 0)
            it, status = b.get_iters()
            assert np.all(status == rp.ST_CONVERGED), name
            x = it[np.argsort(b.slot_map())].astype(np.int64).reshape(-1, 64)
            idle = 1.0 - x.sum() / (x.max(axis=1).sum() * 64.0)
            y = it.astype(np.int64).reshape(-1, 64)
            report.append("%s %.3f (problem order %.3f)" % (name, idle, 1.0 - y.sum() / (y.max(axis=1).sum() * 64.0)))
            assert idle <= 0.03, (name, idle)
    print("idle lane-steps of the gated solve, states through set_state: " + "; ".join(report))


@pytest.mark.parametrize("variant,dtype", [(rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F3, rp.DTYPE_F32_STATE), (rp.VARIANT_F4, rp.DTYPE_F32)])
def test_gated_solve_in_rounds_in_the_other_variants_and_number_modes(oracle, variant, dtype):
    # the same statement for F4 (which never converges: every problem runs into the step budget, all lanes alike) and the fp32 modes,
    # with non-zero end velocities in half of the problems (the general kernels)
    n = 8 * 1024 + 5
    rng = np.random.default_rng(99)
    p0, p1, p2 = rp.problems.generate(515, 0, n, rp.problems.DIST_MONOTONE)
    st0 = oracle.batch_init_feasible(variant, p0, p1, p2)
    m = 8 if variant == rp.VARIANT_F3 else 4
    st0[:, 3:3 + m] = 10.0 ** rng.uniform(-2, 1, (n, 1))
    st0[::2, 3 + m + 1] = 0.25                     # vel0X of every second problem
    out = []
    for rounds in (-1, 4):
        with rp.Batch(n, variant, dtype) as b:
            b.set_params(handoff_rounds=rounds, handoff_lanes=16)
            b.set_state(st0)
            b.solve(1e-8, 40, 0)
            out.append((b.get_state(), b.get_iters()))
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True) and np.array_equal(out[0][1][0], out[1][1][0]) and np.array_equal(out[0][1][1], out[1][1][1])


@pytest.mark.parametrize("dtype", [rp.DTYPE_F32_STATE, rp.DTYPE_F32])
def test_f4_fused_launch_parks_its_fixed_points_and_stores_what_single_steps_store(dtype):
    # Round 6: in a fused fixed-step launch of F4 on an fp32 state a problem whose step has left its stored state bit for bit
    # unchanged takes no further steps (run_lane, PARK: the step is a function of the stored state, so every further step would
    # store the same bits again -- F4's stuck problems, ~52 residual halvings per step for nothing).  Single-step launches cannot
    # park (nothing is carried from launch to launch): 50 of them must leave exactly what one launch of 50 leaves, and the run must
    # really contain fixed points (one more single step changes nothing for them), in fused launches of several lengths.
    n = 64 * 1024 + 13
    p0, p1, p2 = rp.problems.generate(6021, 0, n, rp.problems.DIST_MONOTONE)
    with rp.Batch(n, rp.VARIANT_F4, dtype) as a, rp.Batch(n, rp.VARIANT_F4, dtype) as b, rp.Batch(n, rp.VARIANT_F4, dtype) as c:
        for x in (a, b, c):
            x.set_problems(p0, p1, p2)
        a.step(50)
        for _ in range(50):
            b.step(1)
        for k in (7, 30, 13):
            c.step(k)
        sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
        assert np.all(np.isfinite(sa))
        assert np.array_equal(sa, sb) and np.array_equal(sa, sc)
        assert np.all(a.get_iters()[0] == 50)
        b.step(1)
        fixed = np.all(b.get_state() == sb, axis=1)
        a.step(20)                                   # a second fused launch from the state the first one left: parks them at once
        for _ in range(19):
            b.step(1)
        assert np.array_equal(a.get_state(), b.get_state())
    print("F4 dtype %d: %d of %d problems sit on a fixed point of the step after 50 steps (%.2f %%)" % (dtype, fixed.sum(), n, 100.0 * fixed.mean()))
    if dtype == rp.DTYPE_F32_STATE:      # (the mode that parks; pure fp32 runs the plain loop and is here for the same bit-for-bit statement)
        assert fixed.sum() > n // 200      # ~2.4 % on the benchmark distribution with fp64 arithmetic (oracle, profiles/r6_tuning.md)


@pytest.mark.parametrize("dist,steps", [(rp.problems.DIST_MONOTONE, 50), (rp.problems.DIST_NON_MONOTONE, 30)])
def test_f3_line_search_decisions_through_the_post_convergence_regime_are_the_oracles_or_certified_ties(oracle, dist, steps):
    # ADVICE r4 / VERDICT r4 next 3: beyond step ~19 F3's fixed-step launches search on affine pieces against their own value at
    # s = 0 and count certain failures in closed form (newton_step_inplace<FROZEN>) -- and until this round only x and the
    # multipliers were compared there.  Here every step of a fixed-step run, 1 .. `steps`, is taken from the ORACLE's state before
    # that step, and both halving counts of every problem are the oracle's (onedpath_ip.cpp:927, :944) -- or the oracle's own test
    # values at the first trial decided differently lie within rounding of each other (a certified tie, in units of what a one-ulp
    # move of one input changes: parity_util.certify_line_search_decisions; anything else fails).  Also: the counts' totals where
    # they are comparable, and the step itself at 1e-10.
    n = 2048
    p0, p1, p2 = rp.problems.generate(27182, 0, n, dist)
    aos = oracle.batch_init_feasible(3, p0, p1, p2)
    info = StepInfo()
    diffs_f = diffs_r = tot_gpu = tot_orc = 0
    worst_f = worst_r = 0.0
    late = 0
    with rp.Batch(n) as a:
        for s in range(steps):
            before = aos.copy()
            a.set_state(aos)
            nf, nr = a.step_counted(1)
            got = a.get_state()
            of, orr = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            for i in range(n):
                oracle.step(3, aos[i], info)
                of[i], orr[i] = info.feas_halvings, info.resid_halvings
            cert = certify_line_search_decisions(oracle, 3, before, nf, nr, of, orr)
            diffs_f += cert["feas_diffs"]
            diffs_r += cert["resid_diffs"]
            # the certificates alone would let ANY number of ties pass.  Where the calibration run saw none -- sixteen seeds,
            # profiles/r5_decision_margins.log: the first differing decision comes at step 20 (monotone) / 18 (non-monotone), when the first
            # problems reach the last bit of their limits -- none is allowed (two steps of margin), and past that point a coarse ceiling
            # per step backs the certificates up (calibrated plateaus: 78 % of the problems decide a feasibility trial differently, 25 % a
            # residual trial; a regression that pushed those towards 100 % would be a different kernel, not a rounding).
            quiet = 17 if dist == rp.problems.DIST_MONOTONE else 15
            if s + 1 <= quiet:
                assert cert["feas_diffs"] == 0 and cert["resid_diffs"] == 0, (s + 1, cert["feas_diffs"], cert["resid_diffs"])
            assert cert["feas_diffs"] <= (85 * n) // 100 and cert["resid_diffs"] <= (35 * n) // 100, (s + 1, cert["feas_diffs"], cert["resid_diffs"])
            worst_f, worst_r = max(worst_f, cert["worst_feas"]), max(worst_r, cert["worst_resid"])
            same_f = nf == of                                       # (a feasibility tie sends the two residual searches down different step lengths)
            tot_gpu += int(nr[same_f].sum())
            tot_orc += int(orr[same_f].sum())
            late += int((orr >= 40).sum())
            assert serr(got[:, :3], aos[:, :3]) < TOL, s            # one step from the same state: the iterate itself
    print("F3 dist %d: %d problem-steps through the post-convergence regime (%d with 40+ residual halvings): feasibility decisions that "
          "differ %d (certified ties, worst %.2f of the allowance), residual %d (worst %.2f); residual halvings where the feasibility counts "
          "agree: device %d, oracle %d" % (dist, n * steps, late, diffs_f, worst_f, diffs_r, worst_r, tot_gpu, tot_orc))
    # Past convergence the iterate sits ON its active limits (|a| = L to the last bit): whether x + s dx -- by then x itself --
    # passes `error > 0` is decided by the last bit of a - L, which the device's reciprocal-based evaluation and the reference's
    # divisions round differently for most problems (~75 % of the problem-steps from step ~25 on: each one a certified tie).  A
    # side that finds x infeasible by an ulp walks all 100 halvings and leaves the state where it is; the other moves the
    # multipliers by 1e-16: the same state to rounding, asserted above at 1e-10.
    # (The totals are printed, not compared: ONE tie at the first residual trial -- accepted at once on one side, ~50 halvings on the
    # other -- moves a problem's count by fifty, so totals say nothing that the per-decision certificates do not.)
    assert late > (n * steps) // 4 if dist == rp.problems.DIST_MONOTONE else True      # the regime was reached


def test_f4_pure_fp32_decisions_against_fp32_state_and_a_bound_for_every_problem_that_decides_alike(golden_dir):
    # VERDICT r4 missing 4 / weak 1b: pure fp32 arithmetic had a statistical bound only.  One step from the 4,096 golden
    # fp32-representable states in both modes: RP_DTYPE_F32_STATE (fp64 arithmetic: every problem within 1e-7 of the fp64 oracle,
    # test above) and RP_DTYPE_F32.  Where BOTH halving counts of a problem agree, the two took the same line-search decisions
    # and differ by single-precision arithmetic of the direction alone: those problems are bounded PER PROBLEM; the others
    # ("flipped": an Armijo or feasibility decision below fp32 resolution went the other way, SURVEY C5 / DESIGN section 4) are counted
    # and reported, and their share is bounded.
    t = np.load(os.path.join(golden_dir, "f4_steps.npz"))
    n = len(t["state_in"])
    with rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32_STATE) as a, rp.Batch(n, rp.VARIANT_F4, rp.DTYPE_F32) as b:
        a.set_state(t["state_in"])
        b.set_state(t["state_in"])
        nfa, nra = a.step_counted(1)
        nfb, nrb = b.step_counted(1)
        sa, sb = a.get_state(), b.get_state()
    alike = (nfa == nfb) & (nra == nrb)
    err = np.max(np.abs(sb[:, :3] - sa[:, :3]) / np.maximum(np.abs(sa[:, :3]), 1.0), axis=1)
    flipped = float((~alike).mean())
    print("pure fp32 against fp32 state + fp64 arithmetic, one step from %d states: %.2f %% of the problems take another line-search decision; "
          "the others differ by at most %.2e (median %.1e, 99 %% %.1e); the flipped ones by at most %.2e"
          % (n, 100 * flipped, err[alike].max(), np.median(err[alike]), np.quantile(err[alike], 0.99), err[~alike].max() if flipped else 0.0))
    assert np.all(np.isfinite(sb))
    assert flipped < 0.10
    assert err[alike].max() < F32_ALIKE_TOL


# ---------------------------------------------------------------- round 4: sweeps that were hand-run scripts, now in the suite
def test_fuzz_131072_fresh_gated_solves_against_the_oracle(oracle):
    # tests/checks/fuzz_parity.py (1.44 M solves, hand-run) in suite size: 131,072 fresh problems of each distribution, a seed no
    # other test uses -- iteration counts (certified ties printed), (v, t0, t1) at 1e-10, multipliers where they are determined,
    # and 12 ungated steps of the same problems
    n = 131072
    ties_total = 0
    with rp.Batch(n) as b:
        for dist in (rp.problems.DIST_MONOTONE, rp.problems.DIST_REFERENCE_LIKE, rp.problems.DIST_NON_MONOTONE):
            p0, p1, p2 = rp.problems.generate(70_000_133 + 1_000_003 * dist, 0, n, dist)
            init = oracle.batch_init_feasible(3, p0, p1, p2)
            ref = init.copy()
            it_o, _ = oracle.batch_solve_gated(3, ref, 1e-8, 200, threads=0)
            b.set_problems(p0, p1, p2)
            b.solve(1e-8, 200, 0)
            it_g, st = b.get_iters()
            x = b.get_state()
            ties = certify_iteration_counts(oracle, 3, init, it_g, it_o, 1e-8, max_ties=3)
            ok = keep_mask(n, ties)
            ties_total += len(ties)
            assert np.all(st == rp.ST_CONVERGED)
            assert serr(x[ok, :3], ref[ok, :3]) < TOL
            assert lam_err(x[ok, 3:11], ref[ok, 3:11]) < (LAM_TOL_DEGENERATE if dist == rp.problems.DIST_NON_MONOTONE else LAM_TOL)
            fx = init.copy()
            oracle.batch_steps(3, fx, 12, threads=0)
            b.restart()
            b.step(12)
            assert serr(b.get_state()[:, :3], fx[:, :3]) < TOL
    print("fuzz: 3 x %d fresh solves, %d certified gate tie(s), 0 other iteration mismatches" % (n, ties_total))


@pytest.mark.parametrize("dtype", [rp.DTYPE_F64, rp.DTYPE_F32_STATE])
def test_f4_feasibility_decisions_step_by_step_from_the_oracles_states(oracle, dtype):
    # tests/checks/f4_screen_check.py in suite size: 10 steps (steps 18..27 of the oracle's trajectories, where half of the problems
    # sit in a sequence of 10-19 feasibility halvings) of 4,096 problems, the device re-started from the ORACLE's state before every
    # step (F4 is chaotic).  The stepping launch (k_newton_stream16, with the closed-form ray proof and the per-trial proof) must
    # equal the counted launch (k_newton_counted: in double arithmetic it has NEITHER proof -- every trial is evaluated) bit for
    # bit, and the counted launch's feasibility halvings must be the oracle's, problem by problem.
    n, first_step, steps = 4096, 18, 10
    p0, p1, p2 = rp.problems.generate(31415, 0, n, rp.problems.DIST_MONOTONE)
    aos = oracle.batch_init_feasible(rp.VARIANT_F4, p0, p1, p2)
    oracle.batch_steps(rp.VARIANT_F4, aos, first_step, threads=0)
    info = StepInfo()
    tot_f = long_seq = bad_f = bad_r = 0
    worst = 0.0
    with rp.Batch(n, rp.VARIANT_F4, dtype) as a, rp.Batch(n, rp.VARIANT_F4, dtype) as b:
        for s in range(steps):
            if dtype != rp.DTYPE_F64:
                aos[:] = aos.astype(np.float32).astype(np.float64)      # what the batch will hold (state and constants)
            before = aos.copy()
            a.set_state(aos)
            b.set_state(aos)
            nf, nr = a.step_counted(1)
            b.step(1)
            assert np.array_equal(a.get_state(), b.get_state()), s       # proofs on == every trial evaluated
            of, orr = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            for i in range(n):
                oracle.step(rp.VARIANT_F4, aos[i], info)
                of[i], orr[i] = info.feas_halvings, info.resid_halvings
            tot_f += int(of.sum())
            long_seq += int((of >= 10).sum())
            bad_f += int((nf != of).sum())
            # every residual count that differs is a certified tie: the oracle's own test value within RESID_TIE one-ulp spreads
            # of its threshold at the first trial decided differently (no budget for "last-bit decisions")
            cert = certify_line_search_decisions(oracle, rp.VARIANT_F4, before, nf, nr, of, orr)
            bad_r += cert["resid_diffs"]
            worst = max(worst, cert["worst_resid"])
    print("F4 dtype %d: %d problem-steps, %d feasibility halvings, %d sequences of ten or more; feasibility counts that differ: %d, residual: %d "
          "(every one a certified tie, worst %.2f of the allowance)" % (dtype, n * steps, tot_f, long_seq, bad_f, bad_r, worst))
    assert long_seq > n * steps // 8 and bad_f == 0


@pytest.mark.parametrize("dtype", [rp.DTYPE_F64, rp.DTYPE_F32_STATE, rp.DTYPE_F32])
def test_f4_steps_from_points_that_are_infeasible_beyond_doubt(oracle, dtype):
    # the closed-form count of proven feasibility halvings (skip_certain_halvings) bisects over "g(s 2^-k) > 0", which is
    # monotone in k only if g(0) <= 0 or g is concave.  From a point x that is ITSELF beyond doubt infeasible (a nudge, a set
    # state, an RP_ST_INFEASIBLE start) a convex g can be positive at s, negative in between and positive again near 0: the
    # bisection then "proved" all 100 halvings where the reference halves once or twice and moves.  Starts with zero end
    # velocities (the instantiations that carry the proofs), pushed outside: durations shortened, velocities spread.
    n = 8192
    rng = np.random.RandomState(77)
    p0, p1, p2 = rp.problems.generate(1234, 0, n, rp.problems.DIST_MONOTONE)
    aos = oracle.batch_init_feasible(rp.VARIANT_F4, p0, p1, p2)
    aos[:, 1] *= rng.uniform(0.55, 1.0, n)
    aos[:, 2] *= rng.uniform(0.55, 1.0, n)
    aos[:, 0] = rng.uniform(-120, 260, n)
    aos[0, :3] = (190.0, 2.4, aos[0, 2])                                 # the advisor's example: g = 10 - 140 s + 200 s^2 along (dv, d0) = (-150, 1)
    if dtype != rp.DTYPE_F64:
        aos[:] = aos.astype(np.float32).astype(np.float64)
    outside = np.array([not oracle.satisfied(rp.VARIANT_F4, row) for row in aos])
    assert outside.sum() > n // 2
    info = StepInfo()
    exp = aos.copy()
    of = np.zeros(n, dtype=np.int64)
    for i in range(n):
        oracle.step(rp.VARIANT_F4, exp[i], info)
        of[i] = info.feas_halvings
    with rp.Batch(n, rp.VARIANT_F4, dtype) as a, rp.Batch(n, rp.VARIANT_F4, dtype) as b, rp.Batch(n, rp.VARIANT_F4, dtype) as c:
        a.set_state(aos)
        b.set_state(aos)
        c.set_state(aos)
        nf, _ = a.step_counted(1)
        b.step(1)                                                        # k_newton_stream16, ZV: ray proof + per-trial proof
        c.step(2)                                                        # k_steps_chunks: the same proofs in the fused launch
        b1 = b.get_state()
        b.step(1)
        assert np.array_equal(c.get_state(), b.get_state())
        if dtype != rp.DTYPE_F32:
            # double arithmetic: the counted launch evaluates every trial; the stepping launch must agree bit for bit, and the
            # feasibility counts are the oracle's (fp32 state: the oracle steps from the same fp32-representable point)
            assert np.array_equal(a.get_state(), b1)
            assert np.array_equal(nf, of), "%d feasibility counts differ" % int((nf != of).sum())
        else:
            # single precision decides a borderline trial differently now and then, never by much: no step may collapse to
            # s 2^-100 where the reference moves
            assert np.mean(nf == of) > 0.97 and np.max(np.abs(nf.astype(np.int64) - of)[of < 90]) <= 3
    # where the reference's step moves the point, so does the device's (a step that collapsed to s 2^-100 leaves x where it was)
    moved = np.abs(exp[:, :3] - aos[:, :3]).max(axis=1) > 1e-9
    got_moved = np.abs(b1[:, :3] - aos[:, :3]).max(axis=1) > 1e-9
    assert moved.sum() > 500 and (moved & outside).sum() > 50      # (most starts this far outside stay frozen: 100 halvings, as in the reference)
    assert np.mean(moved == got_moved) > (0.99 if dtype == rp.DTYPE_F32 else 0.9999), np.mean(moved == got_moved)


def test_f4_closed_form_halving_count_on_the_states_where_it_was_unsound(oracle, golden_dir):
    # The regression fixture for the case above: 31 F4 states (fp32-representable rows; inputs only) found in round 4 among 12.6 M
    # perturbed trajectory states, at which round 3's closed form -- which took g to be monotone along the ray -- counted halvings
    # the reference does not make: x beyond doubt infeasible, g convex along the ray, positive at s and near 0, negative in between
    # (this test failed against a library built with that form: profiles/r4_ray_ab.log).  With the monotonicity condition the
    # stepping launches equal the launch that evaluates every trial, bit for bit, and its feasibility counts are the oracle's.
    states = np.load(os.path.join(golden_dir, "f4_ray_cases.npz"))["states"]
    m = len(states)
    assert m == 31 and np.array_equal(states, states.astype(np.float32).astype(np.float64))
    n = 64 * 8                                                           # the cases spread over several waves, padded with a feasible state
    pad = oracle.batch_init_feasible(rp.VARIANT_F4, np.zeros(1), np.full(1, 200.0), np.full(1, 400.0))[0]
    pad = pad.astype(np.float32).astype(np.float64)
    aos = np.tile(pad, (n, 1))
    at = (np.arange(m) * 16 + 3) % n
    aos[at] = states
    info = StepInfo()
    exp = aos.copy()
    of = np.zeros(n, dtype=np.int64)
    for i in range(n):
        oracle.step(rp.VARIANT_F4, exp[i], info)
        of[i] = info.feas_halvings
    assert np.all(of[at] >= 1) and np.all(of[at] < 20)                   # the reference halves a few times and moves
    for dtype in (rp.DTYPE_F32_STATE, rp.DTYPE_F32):
        with rp.Batch(n, rp.VARIANT_F4, dtype) as a, rp.Batch(n, rp.VARIANT_F4, dtype) as b, rp.Batch(n, rp.VARIANT_F4, dtype) as c:
            for x in (a, b, c):
                x.set_state(aos)
            nf, _ = a.step_counted(1)
            b.step(1)
            c.step(2)
            b1 = b.get_state()
            b.step(1)
            assert np.array_equal(c.get_state(), b.get_state())
            if dtype == rp.DTYPE_F32_STATE:
                assert np.array_equal(a.get_state(), b1)
                assert np.array_equal(nf, of), (nf[at], of[at])
                assert serr(b1[:, :3], exp.astype(np.float32).astype(np.float64)[:, :3]) < 1e-6
            else:
                assert np.all(np.abs(nf.astype(np.int64) - of) <= 2), (nf[at], of[at])      # single precision: the same walk, last trials may differ
            assert np.all(np.abs(b1[at, :3] - aos[at, :3]).max(axis=1) > 0)          # every case moves (a collapsed step leaves x where it was)


@pytest.mark.parametrize("variant,dtype", [(rp.VARIANT_F3, rp.DTYPE_F64), (rp.VARIANT_F4, rp.DTYPE_F64)])
@pytest.mark.parametrize("backtrack,max_bt", [(0.5, 0), (0.5, 1), (0.5, 3), (0.25, 40), (0.75, 7), (0.5, 100)])
def test_gated_kernel_steps_with_other_line_search_constants_against_the_oracle(oracle, variant, dtype, backtrack, max_bt):
    # the in-place step of the gated kernel (newton_step_inplace) under non-default rp_params -- budgets of 0, 1
    # and 3 halvings, other backtrack factors -- against the oracle taking the same constants (orc_step_params; (0.5, 100) is the
    # reference).  A gate that never closes (tolerance -1e300: no gap is below it) makes the gated launch take exactly k steps.
    n, k = 4096 + 37, 6
    p0, p1, p2 = rp.problems.generate(97, 0, n, rp.problems.DIST_MONOTONE)
    exp = oracle.batch_init_feasible(variant, p0, p1, p2)
    oracle.batch_steps_params(variant, exp, k, backtrack, max_bt, threads=0)
    with rp.Batch(n, variant, dtype) as g, rp.Batch(n, variant, dtype) as f:
        for b in (g, f):
            b.set_params(backtrack=backtrack, max_backtracks=max_bt)
            b.set_problems(p0, p1, p2)
        g.solve(-1e300, k, 0)                        # k gated steps through k_solve_chunks<START> (outside the feasible set a gap can be negative)
        f.step(k)                                    # the fixed-step kernel
        sg, sf = g.get_state(), f.get_state()
        it, status = g.get_iters()
    assert np.all(it == k) and np.all((status & rp.ST_MAXITER) != 0)
    fin = np.all(np.isfinite(exp[:, :3]), axis=1)
    assert fin.mean() > 0.99
    # a budget of 0-3 halvings lets iterates leave the feasible set (the reference would, too): from there on a step is as
    # ill-conditioned as the point is far outside, and F4 is chaotic anyway -- the tight bound is for the well-posed cases
    tol = TOL if (variant == rp.VARIANT_F3 and max_bt >= 40) else 1e-6
    eg = np.abs(sg[fin, :3] - exp[fin, :3]) / np.maximum(np.abs(exp[fin, :3]), 1.0)
    ef = np.abs(sf[fin, :3] - exp[fin, :3]) / np.maximum(np.abs(exp[fin, :3]), 1.0)
    print("variant %d backtrack %g budget %d: gated kernel worst %.2e (median %.1e), fixed-step kernel worst %.2e" % (
        variant, backtrack, max_bt, np.nanmax(eg), np.nanmedian(eg), np.nanmax(ef)))
    assert np.nanquantile(eg, 0.99) < tol and np.nanquantile(ef, 0.99) < tol
    if variant == rp.VARIANT_F3 and max_bt >= 40:
        assert np.nanmax(eg) < TOL and np.nanmax(ef) < TOL
