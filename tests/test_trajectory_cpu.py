"""The trajectory evaluator without a GPU (rp_trajectory_eval / _vjp / _jvp, rp_batch_trajectory_device, trajectory_eval,
min_time_trajectory): the entries exist and refuse bad arguments before any device call, the torch layer checks
its arguments, and the two restatements of tests/trajectory_ref.py -- the definition in longdouble, the kernels' arithmetic and
summation order in float64 -- agree with the oracle's plot data, with central differences and with each other."""
import ctypes
import os
import re

import numpy as np
import pytest

import rocket_path_amd as rp
import trajectory_ref as tr
from end_velocity_ref import velocities
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ENTRIES = ("rp_trajectory_eval", "rp_trajectory_eval_vjp", "rp_trajectory_eval_jvp", "rp_batch_trajectory_device")


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert lib.rp_abi_version() == 7      # new entries only
    for word in ("onedpath_ip.cpp:1065-1088", "Segment rule", "Extrapolation rule", "NaN rule"):
        assert word in header, word
    assert rp.trajectory_eval.__name__ == "trajectory_eval" and rp.min_time_trajectory.__name__ == "min_time_trajectory"


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    no_vel = capi.pointer_table([good, good, good, 0, 0, good, good, good])
    none = capi.pointer_table([0] * 8)
    vp = ctypes.c_void_p
    ev, vj, jv = lib.rp_trajectory_eval, lib.rp_trajectory_eval_vjp, lib.rp_trajectory_eval_jvp
    bad = capi.RP_ERR_INVALID
    # n == 0, k == 0, a huge k
    assert ev(0, None, 0, 4, table, vp(good), vp(good), None, None) == bad and b"positive" in lib.rp_last_error()
    assert ev(0, None, 4, 0, table, vp(good), vp(good), None, None) == bad
    assert ev(0, None, 4, 1 << 31, table, vp(good), vp(good), None, None) == bad and b"2^31" in lib.rp_last_error()
    assert vj(0, None, 0, 4, table, vp(good), None, None, None, table, None) == bad
    assert jv(0, None, 4, 0, table, vp(good), None, None, vp(good), None, None) == bad
    # a NULL required pointer (the end velocities alone may be NULL: those calls fail later, for want of an output)
    assert ev(0, None, 4, 4, None, vp(good), vp(good), None, None) == bad
    assert ev(0, None, 4, 4, table, None, vp(good), None, None) == bad and b"d_tau" in lib.rp_last_error()
    for f in range(8):
        entries = [good] * 8
        entries[f] = 0
        st = ev(0, None, 4, 4, capi.pointer_table(entries), vp(good), None, None, None)
        assert st == bad
        assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), f
    assert ev(-1, None, 4, 4, table, vp(good), vp(good), None, None) == bad
    # all outputs NULL
    assert ev(0, None, 4, 4, no_vel, vp(good), None, None, None) == bad and b"no output" in lib.rp_last_error()
    assert vj(0, None, 4, 4, table, vp(good), vp(good), None, None, none, None) == bad and b"no output" in lib.rp_last_error()
    assert vj(0, None, 4, 4, table, vp(good), vp(good), None, None, None, None) == bad
    assert jv(0, None, 4, 4, table, vp(good), table, vp(good), None, None, None) == bad and b"no output" in lib.rp_last_error()
    # a misaligned per-query buffer
    assert ev(0, None, 4, 4, table, vp(odd), vp(good), None, None) == bad and b"16-byte" in lib.rp_last_error()
    assert ev(0, None, 4, 4, table, vp(good), None, vp(odd), None) == bad and b"16-byte" in lib.rp_last_error()
    assert vj(0, None, 4, 4, table, vp(good), None, vp(odd), None, table, None) == bad and b"16-byte" in lib.rp_last_error()
    assert vj(0, None, 4, 4, table, vp(good), None, None, None, table, vp(odd)) == bad
    assert jv(0, None, 4, 4, table, vp(good), table, vp(odd), vp(good), None, None) == bad
    assert jv(0, None, 4, 4, table, vp(good), table, None, None, None, vp(odd)) == bad
    # the batch entry: a null handle
    assert lib.rp_batch_trajectory_device(None, vp(good), 4, vp(good), None, None) == bad
    with pytest.raises(ValueError):
        capi.pointer_table([good] * 7)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    tau = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_eval(x, x, x, x, x, x, tau)                                    # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_trajectory(x, x, x, tau)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_eval([0.0] * 4, x, x, x, x, x, tau)                            # not a tensor
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.min_time_trajectory(np.zeros(4), x, x, tau)
    # what comes after the device check, on stand-ins that only claim to be on a device
    from rocket_path_amd import autograd

    def meta(*shape, dtype=torch.float64):
        t = torch.empty(shape, dtype=dtype, device="meta")
        return t

    class OnDevice:
        """the checks read .device, .dtype, .shape and .dim() only"""
        def __init__(self, t, device=torch.device("cuda", 0)):
            self.t, self.device, self.dtype, self.shape = t, device, t.dtype, t.shape

        def dim(self):
            return self.t.dim()

    real = autograd._check_is_tensor
    autograd._check_is_tensor = lambda name, t, who: None
    try:
        v, m = OnDevice(meta(4)), OnDevice(meta(4, 3))
        args = [v, v, v, v, v, v]
        with pytest.raises(TypeError, match="float64"):
            autograd._check_trajectory(OnDevice(meta(4, dtype=torch.float32)), v, v, v, v, v, m, None, None, "trajectory_eval")
        with pytest.raises(ValueError, match="1-D"):
            autograd._check_trajectory(m, m, m, v, v, v, m, None, None, "trajectory_eval")
        with pytest.raises(ValueError, match="lengths differ"):
            autograd._check_trajectory(v, OnDevice(meta(5)), v, v, v, v, m, None, None, "trajectory_eval")
        for wrong, kind, text in ((OnDevice(meta(5)), ValueError, "shape"), (OnDevice(meta(4, dtype=torch.float32)), TypeError, "float64"),
                                  (OnDevice(meta(4), torch.device("cuda", 1)), TypeError, "ROCm device"), (OnDevice(meta(4), torch.device("cpu")), TypeError, "ROCm device")):
            for at in (3, 4, 5):
                bad = list(args)
                bad[at] = wrong
                with pytest.raises(kind, match=text):
                    autograd._check_trajectory(*bad, m, None, None, "trajectory_eval")
            with pytest.raises(kind, match=text):
                autograd._check_trajectory(*args, m, wrong, None, "trajectory_eval")
        for wrong, kind in ((OnDevice(meta(3, 3)), ValueError), (OnDevice(meta(4, 0)), ValueError), (OnDevice(meta(0)), ValueError),
                            (OnDevice(meta(4, 3, 2)), ValueError), (OnDevice(meta(4, 3, dtype=torch.float32)), TypeError),
                            (OnDevice(meta(4, 3), torch.device("cpu")), TypeError)):
            with pytest.raises(kind, match="tau"):
                autograd._check_trajectory(*args, wrong, None, None, "trajectory_eval")
        assert autograd._check_trajectory(*args, m, None, None, "trajectory_eval") is m
    finally:
        autograd._check_is_tensor = real


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families(oracle):
    """name -> spline: per generator a solved family with end velocities (kappa = 0.1, the oracle's gated solve) and, once, random
    unsolved states."""
    from end_velocity_ref import start_state
    out = {}
    for dist in range(3):
        st = start_state(*velocities(oracle, dist, 0.1, 96, 77 + dist))
        oracle.batch_solve_gated(3, st, 1e-8, 200)
        ok = np.isfinite(st[:, :3]).all(axis=1) & (st[:, 1] > 0) & (st[:, 2] > 0)
        assert ok.mean() > 0.9
        out["solved%d" % dist] = (st[ok], tr.spline_of_state(st[ok]))
    out["random"] = (None, tr.random_states(96, 5))
    return out


def test_float64_restatement_equals_the_oracles_plot_data(oracle, families):
    """At tau = h j / 32 the evaluator's arithmetic gives drawSegment's 33 positions per segment and the four end accelerations within
    1e-13, scale-aware.  Asserted on all three generators: with section 13's scales (max(X, 1) for positions, max(X / tmin^2, 1) for
    accelerations, X the size of the spline's terms) against Oracle.sample; with the element's own size, max(|ref|, 1) -- the measure
    of k_sample's parity test (tests/test_gpu_parity.py::test_sample_against_oracle, monotone problems) -- against the longdouble
    definition; and with that measure against Oracle.sample within 1e-13 plus the oracle's own distance from longdouble, which itself
    must be below 1e-13.  On the monotone and the reference-like generator the last bound is 1e-13 alone.  On the non-monotone stress
    generator the positions reach 489 and a sample can pass through 0.28: there the oracle is 8.3e-14 from longdouble by element (this
    arithmetic 7.3e-14) -- two float64 sums whose terms are 489, one ulp of which is 5.7e-14 -- and the two are 1.14e-13 apart."""
    by_element = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1.0)))      # noqa: E731
    for name in ("solved0", "solved1", "solved2"):
        st, sp = families[name]
        d0, d1 = sp[6][:, None], sp[7][:, None]
        j = np.arange(33)[None, :]
        tau = np.concatenate([d0 * (j / 32.0), d0 + d1 * (j / 32.0)], axis=1)
        tau[:, 32] = np.nextafter(sp[6], 0.0)                         # the end of segment 0, on segment 0's side
        pos, _, acc = tr.forward_f64(sp, tau)
        ends = [0, 32, 33, 65]
        ref = [oracle.sample(3, row) for row in st]
        p, a = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        sc = tr.scales(sp)
        scaled = max(float(np.max(np.abs(pos - p) / sc[0])), float(np.max(np.abs(acc[:, ends] - a) / sc[2])))
        element = max(by_element(pos, p), by_element(acc[:, ends], a))
        exact = tr.forward_ld(sp, tau)
        against_ld = max(by_element(pos, exact[0]), by_element(acc[:, ends], exact[2][:, ends]))
        oracle_ld = max(by_element(p, np.asarray(exact[0], dtype=np.float64)), by_element(a, np.asarray(exact[2][:, ends], dtype=np.float64)))
        print("%s against Oracle.sample: %.2e by section 13's scales, %.2e by element; by element against longdouble: this %.2e, the oracle %.2e"
              % (name, scaled, element, against_ld, oracle_ld))
        assert scaled < 1e-13 and against_ld < 1e-13 and oracle_ld < 1e-13, name
        assert element < 1e-13 + (oracle_ld if name == "solved2" else 0.0), name


def _cotangents(n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, k)) for _ in range(3)]


@pytest.mark.parametrize("k", [1, 33, 200])
def test_longdouble_vjp_against_central_differences(families, k):
    # F = sum gp pos + gv vel + ga acc; step 1e-6 max(|x|, 1) per input: truncation ~ step^2 x third derivatives, rounding
    # ~1e-19 / step -- measured 2.2e-8, bound 1e-6 normwise over the eight spline gradients and over tau's
    worst = 0.0
    for name, (_, sp) in families.items():
        n = len(sp[0])
        tau = tr.query_times(sp, k, 3, exact=False, keep_off_knot=1e-3)
        g = _cotangents(n, k, 11)
        bars, tau_bar = tr.vjp_ld(sp, tau, *g)

        def F(spl, t):
            pos, vel, acc = tr.forward_ld(spl, t)
            return g[0] * pos + g[1] * vel + g[2] * acc

        fd = []
        for f in range(8):
            h = LD(1e-6) * np.maximum(np.abs(sp[f]), 1.0).astype(LD)
            up, dn = [np.asarray(a, dtype=LD) for a in sp], [np.asarray(a, dtype=LD) for a in sp]
            up[f] = up[f] + h
            dn[f] = dn[f] - h
            fd.append(np.sum(F(up, tau) - F(dn, tau), axis=1) / (2 * h))
        ht = LD(1e-6) * np.maximum(np.abs(tau), 1.0).astype(LD)
        fd_tau = (F(sp, tau.astype(LD) + ht) - F(sp, tau.astype(LD) - ht)) / (2 * ht)
        err = max(float(np.max(tr.normwise(bars, fd))), float(np.max(tr.normwise([tau_bar], [fd_tau]))))
        worst = max(worst, err)
    print("k = %d: longdouble VJP against central differences, normwise %.2e" % (k, worst))
    assert worst < 1e-6


@pytest.mark.parametrize("k", [1, 2, 33, 64, 200])
def test_duality_and_the_float64_restatements(families, k):
    worst_dual = worst_v = worst_j = 0.0
    for name, (_, sp) in families.items():
        n = len(sp[0])
        tau = tr.query_times(sp, k, 4)
        g = _cotangents(n, k, 12)
        rng = np.random.default_rng(13)
        dots = [rng.standard_normal(n) for _ in range(8)]
        tdot = rng.standard_normal((n, k))
        bars, tau_bar = tr.vjp_ld(sp, tau, *g)
        outs = tr.jvp_ld(sp, tau, dots, tdot)
        # <g, J u> = <J^T g, u> within 1e-15 of the sum of |terms|, in longdouble (64-bit mantissa: eps 1.1e-19 per term)
        left = [np.sum(gi.astype(LD) * oi, axis=1) for gi, oi in zip(g, outs)]
        right = [b * np.asarray(d, dtype=LD) for b, d in zip(bars, dots)] + [np.sum(tau_bar * tdot.astype(LD), axis=1)]
        size = sum(np.sum(np.abs(gi.astype(LD) * oi), axis=1) for gi, oi in zip(g, outs)) + sum(np.abs(r) for r in right[:8]) \
            + np.sum(np.abs(tau_bar * tdot.astype(LD)), axis=1)
        worst_dual = max(worst_dual, float(np.max(np.abs(sum(left) - sum(right)) / size)))
        # the kernels' float64 arithmetic and order against the definition
        b64, t64 = tr.vjp_f64(sp, tau, *g)
        worst_v = max(worst_v, float(np.max(tr.normwise(b64 + [t64], bars + [tau_bar]))))
        worst_j = max(worst_j, float(np.max(tr.normwise(tr.jvp_f64(sp, tau, dots, tdot), outs))))
        pos, vel, acc = tr.forward_f64(sp, tau)
        for got, want, scale in zip((pos, vel, acc), tr.forward_ld(sp, tau), tr.scales(sp)):
            assert float(np.max(np.abs(got - want) / scale)) < 1e-13, name
    print("k = %d: duality %.2e; float64 restatement against longdouble: VJP %.2e, JVP %.2e (normwise)" % (k, worst_dual, worst_v, worst_j))
    assert worst_dual < 1e-15
    assert worst_v < 1e-11 and worst_j < 1e-11      # sanity of the restatement only: the device is held to 10 x what it measures


def test_nan_rule_and_group_order_of_the_restatements():
    sp = tr.random_states(6, 9)
    sp[6][1], sp[7][2], sp[6][3] = 0.0, np.inf, -1.0
    tau = tr.query_times([np.abs(a) for a in sp], 5, 1, exact=False)
    tau[4, 2] = np.nan
    for forward in (tr.forward_ld, tr.forward_f64):
        for out in forward(sp, tau):
            bad = np.isnan(np.asarray(out, dtype=np.float64))
            assert bad[1:4].all() and not bad[0].any() and not bad[5].any()
            assert bad[4, 2] and bad[4].sum() == 1
    assert [tr.group_lanes(k) for k in (1, 2, 3, 33, 64, 65, 200)] == [(1, False), (1, True), (4, False), (64, False), (32, True), (64, False), (64, True)]
