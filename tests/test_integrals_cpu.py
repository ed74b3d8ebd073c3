"""The integrals over time windows without a GPU (rp_trajectory_integrals / _vjp / _jvp, rp_batch_integrals_device, trajectory_integrals,
min_time_integrals): the entries exist and refuse bad arguments before any device call, the torch layer checks its
arguments, and the restatements of tests/integrals_ref.py -- the definition in longdouble, the kernels' arithmetic in float64, the
derivatives with the routing of the window's ends -- agree with a known answer, with Gauss-Legendre quadrature of the evaluator's
definition, with each other and with central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

import crossing_ref as cr
import extrema_ref as xr
import integrals_ref as ir
import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ENTRIES = ("rp_trajectory_integrals", "rp_trajectory_integrals_vjp", "rp_trajectory_integrals_jvp", "rp_batch_integrals_device")
VALUE_BOUND = 1e-12      # of scale x (b - a): 10 x the worst the float64 restatement shows below (6.5e-14), rounded up to a power of ten


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
        comment = header[:header.index("RP_API int %s(" % name)].rsplit("/*", 1)[1]
        assert "replaces" in comment, name      # every entry says what it replaces
    text = header[header.index("How much: the integrals"):]
    for word in ("(pos_int, distance, vel_sq, acc_sq)", "a == b", "monotone pieces", "no antiderivative is differenced", "lo_bar", "no atomics"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # entries only: the revision stays
    assert rp.trajectory_integrals.__name__ == "trajectory_integrals" and rp.min_time_integrals.__name__ == "min_time_integrals"
    assert callable(rp.Batch.integrals_device) and callable(capi.trajectory_integrals) and callable(capi.trajectory_integrals_vjp)
    assert callable(capi.trajectory_integrals_jvp)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    four = capi.integrals_table
    all4, none4 = four([good] * 4), four([0] * 4)
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID
    fwd = lambda n, k, sp, lo, hi, out, dev=0: lib.rp_trajectory_integrals(dev, None, n, k, sp, lo, hi, out)      # noqa: E731
    vjp = lambda n, k, sp, lo, hi, g=all4, bars=table, lb=vp(good), hb=vp(good), dev=0: lib.rp_trajectory_integrals_vjp(      # noqa: E731
        dev, None, n, k, sp, lo, hi, g, bars, lb, hb)
    jvp = lambda n, k, sp, lo, hi, out=all4, dots=table, ld=vp(good), hd=vp(good), dev=0: lib.rp_trajectory_integrals_jvp(      # noqa: E731
        dev, None, n, k, sp, lo, hi, dots, ld, hd, out)
    for call in (lambda *a, **kw: fwd(*a, all4, **kw), vjp, jvp):
        assert call(0, 4, table, vp(good), vp(good)) == bad and b"positive" in lib.rp_last_error()
        assert call(4, 0, table, vp(good), vp(good)) == bad
        assert call(4, 1 << 31, table, vp(good), vp(good)) == bad and b"2^31" in lib.rp_last_error()
        assert call(4, 4, None, vp(good), vp(good)) == bad
        assert call(4, 4, table, vp(good), vp(good), dev=-1) == bad
        assert call(4, 4, table, vp(odd), vp(good)) == bad and b"16-byte" in lib.rp_last_error()
        assert call(4, 4, table, vp(good), vp(odd)) == bad and b"16-byte" in lib.rp_last_error()
        for f in range(8):      # the end velocities alone may be NULL
            entries = [good] * 8
            entries[f] = 0
            if f not in (3, 4):
                assert call(4, 4, capi.pointer_table(entries), None, None) == bad and b"d_spline" in lib.rp_last_error(), f
    # no output asked for; a NULL window end is allowed and gets as far as this
    assert fwd(4, 4, table, None, None, none4) == bad and b"no output" in lib.rp_last_error()
    assert fwd(4, 4, table, vp(good), vp(good), None) == bad and b"no output" in lib.rp_last_error()
    assert fwd(4, 4, capi.pointer_table([good] * 3 + [0, 0] + [good] * 3), None, None, none4) == bad and b"no output" in lib.rp_last_error()
    assert vjp(4, 4, table, None, None, bars=capi.pointer_table([0] * 8), lb=None, hb=None) == bad and b"no output" in lib.rp_last_error()
    assert vjp(4, 4, table, None, None, bars=None, lb=None, hb=None) == bad and b"no output" in lib.rp_last_error()
    assert jvp(4, 4, table, None, None, out=none4) == bad and b"no output" in lib.rp_last_error()
    assert jvp(4, 4, table, None, None, out=None) == bad and b"no output" in lib.rp_last_error()
    for f in range(4):
        one = [good] * 4
        one[f] = odd
        assert fwd(4, 4, table, None, None, four(one)) == bad and b"16-byte" in lib.rp_last_error()
        assert vjp(4, 4, table, None, None, g=four(one)) == bad and b"16-byte" in lib.rp_last_error()
        assert jvp(4, 4, table, None, None, out=four(one)) == bad and b"16-byte" in lib.rp_last_error()
    assert vjp(4, 4, table, None, None, lb=vp(odd)) == bad and vjp(4, 4, table, None, None, hb=vp(odd)) == bad
    assert jvp(4, 4, table, None, None, ld=vp(odd)) == bad and jvp(4, 4, table, None, None, hd=vp(odd)) == bad
    assert lib.rp_batch_integrals_device(None, vp(good), vp(good), 4, all4) == bad
    with pytest.raises(rp.RpError):
        capi.trajectory_integrals(0, 0, 4, 4, [good] * 8, good, good)
    with pytest.raises(rp.RpError):
        capi.trajectory_integrals_vjp(0, 0, 4, 4, [good] * 8, good, good, [good] * 4)
    with pytest.raises(rp.RpError):
        capi.trajectory_integrals_jvp(0, 0, 4, 4, [good] * 8, good, good, [good] * 8)
    with pytest.raises(ValueError, match="four"):
        capi.integrals_table([good] * 3)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_integrals(x, x, x, x, x, x, win, win)                              # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_integrals(x, x, x, win, win)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_integrals([0.0] * 4, x, x, x, x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.min_time_integrals(np.zeros(4), x, x)
    from rocket_path_amd import autograd

    def meta(*shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device="meta")

    class OnDevice:
        """the checks read .device, .dtype, .shape and .dim() only"""
        def __init__(self, t, device=torch.device("cuda", 0)):
            self.t, self.device, self.dtype, self.shape = t, device, t.dtype, t.shape

        def dim(self):
            return self.t.dim()

    stopped = []
    real_check, real_apply, real_solve = autograd._check_is_tensor, autograd._TrajectoryIntegrals.apply, autograd.min_time_solve
    autograd._check_is_tensor = lambda name, t, who: None
    autograd._TrajectoryIntegrals.apply = lambda *a: stopped.append(a) or tuple(range(4))
    autograd.min_time_solve = lambda *a, **kw: stopped.append("solve") or (a[0],) * 5
    try:
        v, m = OnDevice(meta(4)), OnDevice(meta(4, 3))
        args = [v, v, v, v, v, v]
        with pytest.raises(TypeError, match="float64"):
            rp.trajectory_integrals(OnDevice(meta(4, dtype=torch.float32)), v, v, v, v, v, m, m)
        with pytest.raises(ValueError, match="lengths differ"):
            rp.trajectory_integrals(v, OnDevice(meta(5)), v, v, v, v, m, m)
        for wrong, kind, text in ((OnDevice(meta(5)), ValueError, "shape"), (OnDevice(meta(4, dtype=torch.float32)), TypeError, "float64"),
                                  (OnDevice(meta(4), torch.device("cuda", 1)), TypeError, "ROCm device")):
            for at in (3, 4, 5):
                bad = list(args)
                bad[at] = wrong
                with pytest.raises(kind, match=text):
                    rp.trajectory_integrals(*bad, m, m)
            with pytest.raises(kind, match=text):
                rp.trajectory_integrals(*args, vel2=wrong)
        for wrong, kind in ((OnDevice(meta(3, 3)), ValueError), (OnDevice(meta(4, 0)), ValueError), (OnDevice(meta(0)), ValueError),
                            (OnDevice(meta(4, 3, 2)), ValueError), (OnDevice(meta(4, 3, dtype=torch.float32)), TypeError),
                            (OnDevice(meta(4, 3), torch.device("cpu")), TypeError)):
            with pytest.raises(kind, match="lo"):
                rp.trajectory_integrals(*args, wrong, m)
            with pytest.raises(kind, match="hi"):
                rp.trajectory_integrals(*args, None, wrong)
            with pytest.raises(kind, match="min_time_integrals: hi"):      # before the solve: a bad window costs none
                rp.min_time_integrals(v, v, v, m, wrong)
        with pytest.raises(ValueError, match="lo has shape"):
            rp.trajectory_integrals(*args, m, OnDevice(meta(4, 2)))
        assert not stopped
        # good arguments reach the launch in the table's order, the window's ends last; None stays None
        assert rp.trajectory_integrals(*args, m, vel0=v) == tuple(range(4))
        assert len(stopped) == 1 and stopped[0][3] is v and stopped[0][4] is None and stopped[0][8] is m and stopped[0][9] is None
        assert rp.trajectory_integrals(*args)[3] == 3 and stopped[1][8] is None and stopped[1][9] is None
        out = rp.min_time_integrals(v, v, v, m, m)
        assert len(out) == 9 and out[:4] == tuple(range(4)) and stopped[2] == "solve" and len(stopped) == 4
    finally:
        autograd._check_is_tensor, autograd._TrajectoryIntegrals.apply, autograd.min_time_solve = real_check, real_apply, real_solve


# ---------------------------------------------------------------- the restatements
N, K = 512, 8


@pytest.fixture(scope="module")
def families():
    """name -> (spline, lo, hi, the definition's four integrals): random unsolved states, the same with vel0 = vel2 = 0 exactly, the solved
    problems of tests/golden/f3_batch.npz, and extrema_ref.knot_cases' eight with their own windows; each also with the short windows
    (name + "/short")."""
    out = {}
    for name, sp in (("random", tr.random_states(N, 5)), ("rest", cr.rest_to_rest(N, 6)), ("solved", xr.solved_golden(N))):
        lo, hi = xr.windows(sp, K, 21)
        out[name] = (sp, lo, hi, ir.integrals_ld(sp, lo, hi))
        lo, hi = ir.short_windows(sp, K, 22)
        out[name + "/short"] = (sp, lo, hi, ir.integrals_ld(sp, lo, hi))
    sp, lo, hi, _ = xr.knot_cases()
    out["knot"] = (sp, lo, hi, ir.integrals_ld(sp, lo, hi))
    return out


def _of_scale(sp, lo, hi, got, want):
    """Per output the worst |got - want| / (scale x (b - a)) over the queries with a < b."""
    a, b, ok = ir.clamped(sp, lo, hi)
    with np.errstate(all="ignore"):
        W = np.where(ok & (b > a), b - a, LD(1))
        return [float(np.where(ok & (b > a), np.abs(np.asarray(g, dtype=LD) - w) / (s * W), 0).max()) for g, w, s in zip(got, want, ir.value_scales(sp))]


def test_known_answer():
    sp = [np.array([x]) for x in (0.0, 100.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0)]
    want = (100.0, 200.0, 24000.0, 240000.0)      # acc0 = 600, jrk0 = -1200 in segment 0, mirrored in segment 1
    lo, hi = np.array([[-np.inf, 0.0]]), np.array([[np.inf, 1.0]])      # the whole spline, and (0, duration0): exactly half
    for f in (ir.integrals_ld, ir.integrals_f64):
        whole = f(sp)
        both = f(sp, lo, hi)
        for i, w in enumerate(want):
            assert abs(float(whole[i][0, 0]) - w) <= 1e-13 * w and abs(float(both[i][0, 0]) - w) <= 1e-13 * w, (f.__name__, ir.NAMES[i])
            assert abs(float(both[i][0, 1]) - w / 2) <= 1e-13 * w / 2, (f.__name__, ir.NAMES[i])
    half = ir.integrals_f64(sp, lo, hi)
    assert [float(half[i][0, 1]) for i in range(4)] == [w / 2 for w in want]


def test_windows_are_what_they_claim(families):
    for name, (sp, lo, hi, want) in families.items():
        if name == "knot":
            continue
        empty = np.isnan(np.asarray(want[0], dtype=np.float64))
        if name.endswith("/short"):
            T = (sp[6] + sp[7])[:, None]
            assert not empty.any() and ((hi - lo) / T).min() < 1e-8 and ((hi - lo) / T).max() <= 1e-2, name
        else:
            assert 0.002 < empty.mean() < 0.03, (name, empty.mean())      # about 1 % of the windows are empty: the NaN rule


def test_definition_against_gauss_legendre(families):
    """The closed forms against 3-point Gauss-Legendre on the smooth pieces through the evaluator's own definition: exact for these degrees,
    so what is left is longdouble rounding."""
    for name, (sp, lo, hi, want) in families.items():
        gauss = ir.gauss_ld(sp, lo, hi)
        for i in range(4):
            assert np.array_equal(np.isnan(gauss[i]), np.isnan(want[i])), (name, ir.NAMES[i])
        worst = _of_scale(sp, lo, hi, gauss, want)
        print("%-13s the definition against Gauss-Legendre, of scale x (b - a): %s" % (name, " ".join("%.1e" % w for w in worst)))
        assert max(worst) <= 1e-15, (name, worst)


def test_float64_arithmetic_against_the_definition(families):
    overall = 0.0
    for name, (sp, lo, hi, want) in families.items():
        got = ir.integrals_f64(sp, lo, hi)
        a, b, ok = ir.clamped(sp, lo, hi)
        for i in range(4):
            assert got[i].dtype == np.float64 and np.array_equal(np.isnan(got[i]), np.isnan(want[i])), (name, ir.NAMES[i])      # the NaN mask
            assert np.array_equal(np.isnan(got[i]), ~ok), (name, ir.NAMES[i])
            same = ok & (a == b)
            assert np.all(got[i][same] == 0) and not np.signbit(got[i][same]).any(), (name, ir.NAMES[i])      # a == b: exactly +0.0
        worst = _of_scale(sp, lo, hi, got, want)
        overall = max(overall, max(worst))
        print("%-13s the float64 arithmetic against the definition, of scale x (b - a): %s" % (name, " ".join("%.1e" % w for w in worst)))
        assert max(worst) <= VALUE_BOUND, (name, worst)
    print("worst of all: %.2e (asserted: %.0e)" % (overall, VALUE_BOUND))


def test_a_window_of_no_length_is_exactly_zero():
    sp = tr.random_states(16, 3)
    T = sp[6] + sp[7]
    lo = np.stack([0.3 * T, sp[6], T, np.zeros(16), -np.ones(16)], axis=1)
    hi = np.stack([0.3 * T, sp[6], T + 1.0, np.zeros(16), np.zeros(16)], axis=1)
    for f in (ir.integrals_ld, ir.integrals_f64):
        for x in f(sp, lo, hi):
            assert np.all(x == 0) and not np.signbit(np.asarray(x, dtype=np.float64)).any(), f.__name__


def _difference(sp, lo, hi, g, keep):
    """Central differences of sum(g x integrals_ld) over the kept queries in all eight inputs (per problem) and both window ends (per
    query), steps 1e-6 max(|x|, 1)."""
    def loss(spx, lox, hix):
        out = ir.integrals_ld(spx, lox, hix)
        return sum(np.where(keep, LD(1) * x * o, LD(0)) for x, o in zip(g, out))

    fd = []
    for f in range(8):
        h = (1e-6 * np.maximum(np.abs(sp[f]), 1.0)).astype(LD)
        up, dn = [np.asarray(x, dtype=LD) for x in sp], [np.asarray(x, dtype=LD) for x in sp]
        up[f], dn[f] = up[f] + h, dn[f] - h
        fd.append((loss(up, lo, hi).sum(axis=1) - loss(dn, lo, hi).sum(axis=1)) / (2 * h))
    lo, hi = lo.astype(LD), hi.astype(LD)
    with np.errstate(all="ignore"):      # the infinite ends of column 0, which is not kept
        h = (1e-6 * np.maximum(np.abs(lo), 1.0)).astype(LD)
        fd.append(np.where(keep, (loss(sp, lo + h, hi) - loss(sp, lo - h, hi)) / (2 * h), LD(0)))
        h = (1e-6 * np.maximum(np.abs(hi), 1.0)).astype(LD)
        fd.append(np.where(keep, (loss(sp, lo, hi + h) - loss(sp, lo, hi - h)) / (2 * h), LD(0)))
    return fd


def test_reverse_mode_against_central_differences(families):
    rng = np.random.default_rng(31)
    for name in ("random", "rest", "solved"):
        sp, lo, hi, want = families[name]
        keep = ir.kept_for_differences(sp, lo, hi)
        finite = ~np.isnan(np.asarray(want[0], dtype=np.float64))
        share = keep.sum() / finite[:, [0] + list(range(2, K))].sum()      # column 1 is left out, as in section 15
        g = [np.where(keep, rng.standard_normal(lo.shape), 0.0) for _ in range(4)]
        bars, lo_bar, hi_bar = ir.vjp_ld(sp, lo, hi, g)
        fd = _difference(sp, lo, hi, g, keep)
        rows = keep.any(axis=1)
        err = tr.normwise(list(bars) + [lo_bar, hi_bar], fd)[rows]
        print("%-7s reverse mode against central differences: worst %.2e normwise, %.0f %% of the finite queries kept" % (name, err.max(), 100 * share))
        assert share >= 0.5 and err.max() <= 1e-6, (name, share, err.max())


def _random_tangents(sp, lo, rng):
    return [rng.standard_normal(len(sp[0])) for _ in range(8)], rng.standard_normal(lo.shape), rng.standard_normal(lo.shape)


def _zap(xs):
    return [np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x) for x in xs]


def test_duality_of_the_two_modes(families):
    rng = np.random.default_rng(32)
    for name, (sp, lo, hi, _) in families.items():
        g = [rng.standard_normal(lo.shape) for _ in range(4)]
        dots, lo_dot, hi_dot = _random_tangents(sp, lo, rng)
        bars, lo_bar, hi_bar = ir.vjp_ld(sp, lo, hi, g)
        tangent = ir.jvp_ld(sp, lo, hi, dots, lo_dot, hi_dot)
        left = [np.where(np.isnan(d), LD(0), LD(1) * x * d) for x, d in zip(g, tangent)]
        right = [b * d for b, d in zip(bars, dots)] + [lo_bar * lo_dot, hi_bar * hi_dot]
        size = sum(np.abs(x).sum() for x in left + right)
        gap = abs(sum(x.sum() for x in left) - sum(x.sum() for x in right))
        print("%-13s <g, J u> against <J^T g, u>: %.1e of the sum of |terms|" % (name, float(gap / size)))
        assert gap <= 1e-15 * size, name


def test_float64_derivatives_against_longdouble(families):
    """What the GPU test measures the kernels by: the float64 restatements of both modes, in the kernels' arithmetic and the VJP's order of
    additions, against longdouble, normwise per problem."""
    rng = np.random.default_rng(33)
    worst = {"vjp": 0.0, "jvp": 0.0}
    for name, (sp, lo, hi, _) in families.items():
        g = [rng.standard_normal(lo.shape) for _ in range(4)]
        dots, lo_dot, hi_dot = _random_tangents(sp, lo, rng)
        want = ir.vjp_ld(sp, lo, hi, g)
        got = ir.vjp_f64(sp, lo, hi, g)
        v = float(np.max(tr.normwise(list(got[0]) + [got[1], got[2]], list(want[0]) + [want[1], want[2]])))
        j = float(np.max(tr.normwise(_zap(ir.jvp_f64(sp, lo, hi, dots, lo_dot, hi_dot)), _zap(ir.jvp_ld(sp, lo, hi, dots, lo_dot, hi_dot)))))
        print("%-13s float64 against longdouble, normwise: reverse mode %.1e, forward mode %.1e" % (name, v, j))
        worst["vjp"], worst["jvp"] = max(worst["vjp"], v), max(worst["jvp"], j)
    assert worst["vjp"] <= 1e-12 and worst["jvp"] <= 1e-13, worst      # 10 x the measured 3.9e-14 and 4.6e-15, rounded up to a power of ten


def test_none_is_zeros_in_both_modes(families):
    sp, lo, hi, _ = families["random"]
    rng = np.random.default_rng(34)
    g = [rng.standard_normal(lo.shape), None, rng.standard_normal(lo.shape), None]
    z = np.zeros(lo.shape)
    for f in (ir.vjp_ld, ir.vjp_f64):
        a, b = f(sp, lo, hi, g), f(sp, lo, hi, [g[0], z, g[2], z])
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(list(a[0]) + [a[1], a[2]], list(b[0]) + [b[1], b[2]]))
    dots = [rng.standard_normal(N) if f % 2 else None for f in range(8)]
    full = [d if d is not None else np.zeros(N) for d in dots]
    for f in (ir.jvp_ld, ir.jvp_f64):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(f(sp, lo, hi, dots, None, z), f(sp, lo, hi, full, z, z)))


def test_routing_exactly(families):
    rng = np.random.default_rng(35)
    for name in ("random", "rest", "solved"):
        sp = families[name][0]
        n = len(sp[0])
        g = [rng.standard_normal((n, 1)) for _ in range(4)]
        for f, T in ((ir.vjp_ld, LD), (ir.vjp_f64, np.float64)):
            # the whole spline: both ends are clamps, nothing reaches lo or hi; the END term f(duration1) sits on duration1, the knot's
            # f0(duration0) on duration0, each next to what segment_chain puts there
            bars, lo_bar, hi_bar = f(sp, None, None, g)
            assert np.all(lo_bar == 0) and np.all(hi_bar == 0), name
            terms, _, _ = ir._terms(sp, None, None, g, T)
            chain = ir._chain(sp, terms.sum(axis=2)[:8], T)
            core = ir._core(sp, None, None, T)
            weigh = lambda which, seg: sum(np.asarray(x, dtype=T) * core["seg"][seg][which][i] for i, x in enumerate(g))[:, 0]      # noqa: E731
            with np.errstate(all="ignore"):
                for at, seg in ((6, 0), (7, 1)):
                    end = weigh("fb", seg)
                    assert np.abs(end).min() > 0 and np.all(np.abs((bars[at] - chain[at]) - end) <= 1e-9 * (np.abs(end) + np.abs(chain[at]))), (name, at)
            # a window inside segment 0 touches nothing of segment 1
            d0 = np.asarray(sp[6])[:, None]
            a, b = 0.2 * d0, 0.7 * d0
            bars, lo_bar, hi_bar = f(sp, a, b, g)
            assert all(np.all(bars[at] == 0) for at in (2, 4, 7)), name                          # pos2, vel2, duration1
            assert np.abs(lo_bar).min() > 0 and np.abs(hi_bar).min() > 0 and np.abs(bars[6]).min() > 0, name
            # a window inside segment 1: its ends are local times, so what goes to lo and hi leaves duration0 again
            T_ = d0 + np.asarray(sp[7])[:, None]
            a, b = d0 + 0.2 * (T_ - d0), d0 + 0.7 * (T_ - d0)
            bars, lo_bar, hi_bar = f(sp, a, b, g)
            assert all(np.all(bars[at] == 0) for at in (0, 3)), name                             # pos0, vel0
            terms, _, _ = ir._terms(sp, a, b, g, T)
            assert np.array_equal(terms[8][:, 0], -(lo_bar + hi_bar)[:, 0]), name


def test_nan_rule_of_the_restatements():
    sp = [a.copy() for a in tr.random_states(64, 9)]
    lo, hi = xr.windows(sp, 5, 10)
    clean = ir.integrals_f64(sp, lo, hi)
    sp[6][3], sp[7][20], sp[6][40], sp[7][63] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[50, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    bad = np.zeros(lo.shape, dtype=bool)
    bad[[3, 20, 40, 63]] = True
    bad[10, 0] = bad[50, 4] = bad[11, 3] = True
    for f in (ir.integrals_ld, ir.integrals_f64):
        for x, ref in zip(f(sp, lo, hi), clean):
            assert np.array_equal(np.isnan(x), bad | np.isnan(ref)), f.__name__
    got = ir.integrals_f64(sp, lo, hi)
    assert all(np.array_equal(x[~bad], ref[~bad], equal_nan=True) for x, ref in zip(got, clean))
    # a NaN output's gradient counts as zero: lo_bar and hi_bar are 0 there, and the good problems' gradients are finite
    g = [np.ones(lo.shape) for _ in range(4)]
    for f in (ir.vjp_ld, ir.vjp_f64):
        bars, lo_bar, hi_bar = f(sp, lo, hi, g)
        assert np.all(lo_bar[bad] == 0) and np.all(hi_bar[bad] == 0)
        good = np.ones(64, dtype=bool)
        good[[3, 20, 40, 63]] = False
        assert all(np.isfinite(np.asarray(b, dtype=np.float64)[good]).all() and np.isnan(np.asarray(b, dtype=np.float64)[~good]).all() for b in bars)
