"""The evaluator's second derivative without a GPU (rp_trajectory_eval_hvp, trajectory_eval(order=2), min_time_trajectory(order=2);
DESIGN.md section 17): the entry exists and refuses bad arguments before any device call, the torch layer refuses an order that is neither
1 nor 2 before it looks at a device, and the two restatements of tests/trajectory_hvp_ref.py -- the definition in longdouble, the kernel's
arithmetic and summation order in float64 -- agree with central differences of the first-order definition (trajectory_ref.vjp_ld), with
the identities a second derivative must satisfy, and with each other."""
import ctypes
import os
import re

import numpy as np
import pytest

import rocket_path_amd as rp
import trajectory_hvp_ref as hr
import trajectory_ref as tr
from end_velocity_ref import velocities
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
KS = (1, 2, 33, 200)


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    name = "rp_trajectory_eval_hvp"
    assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header)
    assert header.index("RP_API int rp_trajectory_eval_jvp") < header.index("RP_API int " + name) < header.index("RP_API int rp_batch_trajectory_device")
    assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.rp_abi_version() == 7      # a new entry only
    assert callable(capi.trajectory_eval_hvp)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    none = capi.pointer_table([0] * 8)
    vp = ctypes.c_void_p
    hv = lib.rp_trajectory_eval_hvp
    bad = capi.RP_ERR_INVALID
    # a NULL spline table, n == 0, k == 0, a huge k, a bad device
    assert hv(0, None, 4, 4, None, vp(good), vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"d_spline" in lib.rp_last_error()
    assert hv(0, None, 0, 4, table, vp(good), vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"positive" in lib.rp_last_error()
    assert hv(0, None, 4, 0, table, vp(good), vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"positive" in lib.rp_last_error()
    assert hv(0, None, 4, 1 << 31, table, vp(good), vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"2^31" in lib.rp_last_error()
    assert hv(-1, None, 4, 4, table, vp(good), vp(good), None, None, table, vp(good), table, vp(good)) == bad
    # a NULL required pointer: tau, and every entry of the spline table but the end velocities
    assert hv(0, None, 4, 4, table, None, vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"d_tau" in lib.rp_last_error()
    for f in range(8):
        entries = [good] * 8
        entries[f] = 0
        st = hv(0, None, 4, 4, capi.pointer_table(entries), vp(good), None, None, None, None, None, none, None)
        assert st == bad
        assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), f
    # a misaligned n x k pointer, wherever it is
    for at in range(5):
        per_query = [vp(good)] * 5
        per_query[at] = vp(odd)
        g_pos, g_vel, g_acc, tau_dot, tau_bar_dot = per_query
        assert hv(0, None, 4, 4, table, vp(good), g_pos, g_vel, g_acc, table, tau_dot, table, tau_bar_dot) == bad and b"16-byte" in lib.rp_last_error(), at
    assert hv(0, None, 4, 4, table, vp(odd), vp(good), None, None, table, vp(good), table, vp(good)) == bad and b"16-byte" in lib.rp_last_error()
    # all outputs NULL: a table of NULLs, and no table
    assert hv(0, None, 4, 4, table, vp(good), vp(good), None, None, table, vp(good), none, None) == bad and b"no output" in lib.rp_last_error()
    assert hv(0, None, 4, 4, table, vp(good), vp(good), None, None, None, None, None, None) == bad and b"no output" in lib.rp_last_error()


def test_an_order_that_is_neither_1_nor_2_is_refused_before_the_device_checks():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    tau = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"trajectory_eval: order must be 1 or 2, got 3"):
        rp.trajectory_eval(x, x, x, x, x, x, tau, order=3)
    with pytest.raises(ValueError, match=r"min_time_trajectory: order must be 1 or 2, got 0"):
        rp.min_time_trajectory(x, x, x, tau, order=0)
    for order in (1, 2):      # a valid order goes on to the device checks
        with pytest.raises(TypeError, match="ROCm device"):
            rp.trajectory_eval(x, x, x, x, x, x, tau, order=order)
        with pytest.raises(TypeError, match="ROCm device"):
            rp.min_time_trajectory(x, x, x, tau, order=order)


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families(oracle):
    """name -> spline: per generator a solved family with end velocities (kappa = 0.1, the oracle's gated solve) and, once, random
    unsolved states (tests/test_trajectory_cpu.py's)."""
    from end_velocity_ref import start_state
    out = {}
    for dist in range(3):
        st = start_state(*velocities(oracle, dist, 0.1, 96, 77 + dist))
        oracle.batch_solve_gated(3, st, 1e-8, 200)
        ok = np.isfinite(st[:, :3]).all(axis=1) & (st[:, 1] > 0) & (st[:, 2] > 0)
        assert ok.mean() > 0.9
        out["solved%d" % dist] = tr.spline_of_state(st[ok])
    out["random"] = tr.random_states(96, 5)
    return out


@pytest.fixture(scope="module")
def random_1024():
    return tr.random_states(1024, 5)


@pytest.mark.parametrize("k", KS)
def test_longdouble_hvp_against_central_differences_of_the_vjp(random_1024, k):
    # (vjp(x + e v) - vjp(x - e v)) / 2 e at e = 1e-6 along a random direction v of all nine inputs: truncation ~ e^2 x fourth
    # derivatives, rounding ~1e-19 / e -- measured 8.1e-9 (it scales with e^2), bound 1e-6 normwise per problem, the margin of the
    # first-order check (test_trajectory_cpu.py)
    sp = random_1024
    n = len(sp[0])
    tau = tr.query_times(sp, k, 3, exact=False, keep_off_knot=1e-3)
    g = hr.gradients(n, k, 11)
    dots, tdot = hr.directions(n, k, 12)
    bars, tau_bar = hr.hvp_ld(sp, tau, *g, dots, tdot)
    e = LD(1e-6)
    moved = lambda sign: ([np.asarray(a, dtype=LD) + sign * e * np.asarray(d, dtype=LD) for a, d in zip(sp, dots)],      # noqa: E731
                          tau.astype(LD) + sign * e * tdot.astype(LD))
    up, dn = tr.vjp_ld(*moved(+1), *g), tr.vjp_ld(*moved(-1), *g)
    fd = [(a - b) / (2 * e) for a, b in zip(up[0] + [up[1]], dn[0] + [dn[1]])]
    err = float(np.max(tr.normwise(bars + [tau_bar], fd)))
    print("k = %d: longdouble HVP against central differences of the longdouble VJP, normwise %.2e" % (k, err))
    assert err <= 1e-6


@pytest.mark.parametrize("k", KS)
def test_symmetry_translation_and_zero_gradients(random_1024, k):
    sp = random_1024
    n = len(sp[0])
    tau = tr.query_times(sp, k, 4)
    g = hr.gradients(n, k, 13)
    u, v = hr.directions(n, k, 14), hr.directions(n, k, 15)
    # u^T H[g] v = v^T H[g] u within 1e-15 of the sum of |terms|, in longdouble (eps 1.1e-19 per term; 3.2e-18 measured)
    left, size_l = hr.bilinear(*hr.hvp_ld(sp, tau, *g, *v), *u)
    right, size_r = hr.bilinear(*hr.hvp_ld(sp, tau, *g, *u), *v)
    asym = float(np.max(np.abs(left - right) / (size_l + size_r)))
    print("k = %d: symmetry %.2e of the sum of |terms|" % (k, asym))
    assert asym <= 1e-15
    zero = np.zeros((n, k))
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        # the spline moved as a whole: nothing changes
        bars, tau_bar = hvp(sp, tau, *g, hr.translation(n), zero)
        assert all(np.all(np.asarray(b) == 0) for b in bars) and np.all(np.asarray(tau_bar) == 0), hvp.__name__
        # no upstream gradient: no second derivative
        bars, tau_bar = hvp(sp, tau, zero, zero, zero, *v)
        assert all(np.all(np.asarray(b) == 0) for b in bars) and np.all(np.asarray(tau_bar) == 0), hvp.__name__


@pytest.mark.parametrize("k", [1, 2, 33, 64, 200])
def test_float64_restatement_against_longdouble(families, k):
    """The kernel's arithmetic and order against the definition, normwise per problem, on the three solved generator families and the random
    states: the yardstick of the device check (tests/trajectory_hvp_gpu_cases.py holds the device to 10 x what this measures on ITS
    inputs).  Here only its sanity is asserted, at the bound the first-order restatements have (test_trajectory_cpu.py)."""
    worst = {}
    for name, sp in families.items():
        n = len(sp[0])
        tau = tr.query_times(sp, k, 5)
        g = hr.gradients(n, k, 16)
        dots, tdot = hr.directions(n, k, 17)
        bars, tau_bar = hr.hvp_ld(sp, tau, *g, dots, tdot)
        b64, t64 = hr.hvp_f64(sp, tau, *g, dots, tdot)
        worst[name] = float(np.max(tr.normwise(b64 + [t64], bars + [tau_bar])))
    print("k = %d: float64 restatement of the HVP against longdouble, normwise: %s" % (k, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) < 1e-11


def test_nan_rule_of_the_restatements():
    sp = tr.random_states(6, 9)
    sp[6][1], sp[7][2], sp[6][3] = 0.0, np.inf, -1.0
    tau = tr.query_times([np.abs(a) for a in sp], 5, 1, exact=False)
    tau[4, 2] = np.nan      # a query of segment 1: pos0's and vel0's results stay finite, every other one of its problem is NaN
    dots, tdot = hr.directions(6, 5, 2)
    tdot[5, 1] = np.nan
    seg1 = bool(tau[5, 1] >= sp[6][5])
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars, tau_bar = hvp(sp, tau, *hr.gradients(6, 5, 3), dots, tdot)
        bad = np.isnan(np.asarray(tau_bar, dtype=np.float64))
        assert bad[1:4].all() and not bad[0].any()
        assert bad[4, 2] and bad[4].sum() == 1 and bad[5, 1] and bad[5].sum() == 1
        for f, b in enumerate(bars):
            b = np.asarray(b, dtype=np.float64)
            assert np.isnan(b[1:4]).all() and np.isfinite(b[0]), f
            assert np.isnan(b[4]) == (f not in (0, 3)), f
            # a NaN tau_dot poisons the sums of its query's segment: segment 1's reach all but pos0 and vel0, segment 0's all but pos2,
            # vel2 and duration1
            assert np.isnan(b[5]) == (f not in ((0, 3) if seg1 else (2, 4, 7))), f
