"""The tracking integrals' second derivative without a GPU (rp_trajectory_tracking_hvp, trajectory_tracking(order=2),
min_time_tracking(order=2)): the entry exists and refuses bad arguments before any device call, the torch layer
refuses an order that is neither 1 nor 2 before it looks at a device, and the two restatements of tests/tracking_hvp_ref.py -- the
definition in longdouble, the kernel's arithmetic and order of additions in float64 -- agree with central differences of the first-order
definition (tracking_ref.vjp_ld), with the identities a second derivative must satisfy, with section 19's restatement where B stands
still, with a known answer, and with each other.  Families and windows are tests/test_tracking_cpu.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

import extrema_ref as xr
import integrals_hvp_ref as ih
import rocket_path_amd as rp
import tracking_hvp_ref as hr
import tracking_ref as kr
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N, K = 512, 8
F64_BOUND = 1e-12      # normwise per problem: 10 x the worst the float64 restatement shows below (5.2e-14), rounded up to a power of ten
NAME = "rp_trajectory_tracking_hvp"


def _f(x):
    return np.asarray(x, dtype=np.float64)


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+%s\s*\(" % NAME, header)
    assert header.index("RP_API int rp_trajectory_tracking_jvp") < header.index("RP_API int " + NAME) < header.index("RP_API int rp_trajectory_meeting")
    comment = header[:header.index("RP_API int %s(" % NAME)].rsplit("/*", 1)[1]
    for word in ("replaces", "held fixed", "symmetric", "rp_trajectory_tracking_jvp", "one-sided", "same bits", "no atomics", "nineteen"):
        assert word in comment, word
    assert NAME in capi.SIGNATURES and hasattr(lib, NAME)
    assert lib.rp_abi_version() == 7      # a new entry only
    assert callable(capi.trajectory_tracking_hvp)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    none = capi.pointer_table([0] * 8)
    three = capi.tracking_table
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID

    def hv(n=4, k=4, a=table, b=table, lo=vp(good), hi=vp(good), dl=vp(good), g=three([good] * 3), ad=table, bd=table, ld=vp(good), hd=vp(good),
           dd=vp(good), ba=table, bb=table, lb=vp(good), hb=vp(good), db=vp(good), dev=0):
        return lib.rp_trajectory_tracking_hvp(dev, None, n, k, a, b, lo, hi, dl, g, ad, bd, ld, hd, dd, ba, bb, lb, hb, db)

    assert hv(a=None) == bad and b"d_spline_a" in lib.rp_last_error()
    assert hv(b=None) == bad and b"d_spline_b" in lib.rp_last_error()
    assert hv(n=0) == bad and b"positive" in lib.rp_last_error()
    assert hv(k=0) == bad and b"positive" in lib.rp_last_error()
    assert hv(k=1 << 31) == bad and b"2^31" in lib.rp_last_error()
    assert hv(dev=-1) == bad
    nothing = dict(lo=None, hi=None, dl=None, g=None, ad=None, bd=None, ld=None, hd=None, dd=None, ba=none, bb=None, lb=None, hb=None, db=None)
    for f in range(8):      # every required pointer of either table: all entries but the end velocities
        entries = [good] * 8
        entries[f] = 0
        for side in ("a", "b"):
            assert hv(**dict(nothing, **{side: capi.pointer_table(entries)})) == bad
            assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), (side, f)
    # a misaligned n x k pointer, wherever it is
    for name in ("lo", "hi", "dl", "ld", "hd", "dd", "lb", "hb", "db"):
        assert hv(**{name: vp(odd)}) == bad and b"16-byte" in lib.rp_last_error(), name
    for f in range(3):
        one = [good] * 3
        one[f] = odd
        assert hv(g=three(one)) == bad and b"16-byte" in lib.rp_last_error(), f
    # all outputs NULL: tables of NULLs, and no tables
    assert hv(ba=none, bb=none, lb=None, hb=None, db=None) == bad and b"no output" in lib.rp_last_error()
    assert hv(ba=None, bb=None, lb=None, hb=None, db=None) == bad and b"no output" in lib.rp_last_error()
    with pytest.raises(rp.RpError):
        capi.trajectory_tracking_hvp(0, 0, 4, 4, [good] * 8, [good] * 8, good, good, good, [good] * 3, [good] * 8, [good] * 8)


def test_an_order_that_is_neither_1_nor_2_is_refused_before_the_device_checks():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    six = (x, x, x, x, x, x)
    with pytest.raises(ValueError, match=r"trajectory_tracking: order must be 1 or 2, got 3"):
        rp.trajectory_tracking(six, six, win, win, win, order=3)
    with pytest.raises(ValueError, match=r"min_time_tracking: order must be 1 or 2, got 0"):
        rp.min_time_tracking((x, x, x), (x, x, x), win, win, win, order=0)
    for order in (1, 2):      # a valid order goes on to the device checks
        with pytest.raises(TypeError, match="ROCm device"):
            rp.trajectory_tracking(six, six, win, win, win, order=order)
        with pytest.raises(TypeError, match="ROCm device"):
            rp.min_time_tracking((x, x, x), (x, x, x), win, win, win, order=order)


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families():
    return {name: kr.family(name, N, K) for name in kr.FAMILIES}


def test_longdouble_hvp_against_central_differences_of_the_vjp(families):
    """(vjp_ld(x + e d) - vjp_ld(x - e d)) / 2 e at e = 1e-6 along d = max(|x|, 1) x a standard normal in all nineteen inputs, over the
    queries tracking_ref.kept_for_differences keeps, normwise per problem; follower0 sits on the delay-0 kink and is left out, as at first
    order.  Measured: 2.4e-8 random, 6.7e-10 solved, 5.9e-9 follower (truncation); kept 73.1 %, 73.2 %, 98.7 % of the finite queries."""
    e = 1e-6
    for name in ("random", "solved", "follower"):
        a, b, lo, hi, delay = families[name]
        keep = kr.kept_for_differences(a, b, lo, hi, delay)
        finite = ~np.isnan(_f(kr.tracking_ld(a, b, lo, hi, delay)[0]))
        share = keep.sum() / finite.sum()
        rng = np.random.default_rng(41)
        g = [np.where(keep, rng.standard_normal(lo.shape), 0.0) for _ in range(3)]
        a_dot, b_dot, lo_dot, hi_dot, dl_dot = hr.directions(a, b, lo, hi, delay, 42, scaled=True)
        lo_dot, hi_dot, dl_dot = (np.where(keep, x, 0.0) for x in (lo_dot, hi_dot, dl_dot))
        got = hr.hvp_ld(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, dl_dot)

        def moved(sign):
            with np.errstate(all="ignore"):      # the infinite window ends
                return ([x + sign * e * d for x, d in zip(a, a_dot)], [x + sign * e * d for x, d in zip(b, b_dot)], lo + sign * e * lo_dot,
                        hi + sign * e * hi_dot, delay + sign * e * dl_dot)

        up, dn = moved(+1), moved(-1)
        fd = [(x - y) / (2 * LD(e)) for x, y in zip(hr.flat(kr.vjp_ld(*up, g)), hr.flat(kr.vjp_ld(*dn, g)))]
        for at in (16, 17, 18):
            fd[at] = np.where(keep, fd[at], LD(0))
        err = tr.normwise(hr.flat(got), fd)[keep.any(axis=1)]
        print("%-9s longdouble HVP against central differences of the longdouble VJP: worst %.2e normwise; %.1f %% of the finite queries kept"
              % (name, err.max(), 100 * share))
        assert share >= 0.5 and err.max() <= 1e-6, (name, share, err.max())


def test_symmetry(families):
    """u^T H[g] v = v^T H[g] u within 1e-15 of the sum of |terms|, in longdouble."""
    for name, (a, b, lo, hi, delay) in families.items():
        g = hr.gradients(lo.shape, 43)
        u, v = hr.directions(a, b, lo, hi, delay, 44), hr.directions(a, b, lo, hi, delay, 45)
        left, size_l = hr.bilinear(hr.hvp_ld(a, b, lo, hi, delay, g, *v), u)
        right, size_r = hr.bilinear(hr.hvp_ld(a, b, lo, hi, delay, g, *u), v)
        asym = float(np.max(np.abs(left - right) / (size_l + size_r)))
        print("%-9s symmetry %.2e of the sum of |terms|" % (name, asym))
        assert asym <= 1e-15, name


def test_exact_zeros(families):
    for name, (a, b, lo, hi, delay) in families.items():
        n = len(a[0])
        g = hr.gradients(lo.shape, 46)
        v = hr.directions(a, b, lo, hi, delay, 47)
        for hvp in (hr.hvp_ld, hr.hvp_f64):
            # both splines moved together: the gap does not change, so nothing does
            result = hvp(a, b, lo, hi, delay, g, hr.translation(n), hr.translation(n), None, None, None)
            assert all(np.all(np.asarray(x) == 0) for x in hr.flat(result)), (name, hvp.__name__)
            # no upstream gradient: no second derivative
            zero = np.zeros(lo.shape)
            for none in ([zero] * 3, None, [None] * 3):
                assert all(np.all(np.asarray(x) == 0) for x in hr.flat(hvp(a, b, lo, hi, delay, none, *v))), (name, hvp.__name__)


def test_none_is_zeros(families):
    a, b, lo, hi, delay = families["random"]
    rng = np.random.default_rng(48)
    g = [rng.standard_normal(lo.shape), None, rng.standard_normal(lo.shape)]
    z = np.zeros(lo.shape)
    a_dot = [rng.standard_normal(N) if f % 2 else None for f in range(8)]
    b_dot = [None if f % 2 else rng.standard_normal(N) for f in range(8)]
    full = lambda dots: [d if d is not None else np.zeros(N) for d in dots]      # noqa: E731
    ld = rng.standard_normal(lo.shape)
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        x = hvp(a, b, lo, hi, delay, g, a_dot, b_dot, ld, None, None)
        y = hvp(a, b, lo, hi, delay, [g[0], z, g[2]], full(a_dot), full(b_dot), ld, z, z)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(hr.flat(x), hr.flat(y))), hvp.__name__
        x = hvp(a, b, lo, hi, delay, g, None, b_dot, None, None, ld)
        y = hvp(a, b, lo, hi, delay, g, [np.zeros(N)] * 8, full(b_dot), z, z, ld)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(hr.flat(x), hr.flat(y))), hvp.__name__


def test_consistency_with_the_single_spline_integrals():
    """B a constant spline (three equal positions, at rest, T_B > T_A) at a delay of 0: gap_int = pos_int_A - c (b - a) and relvel_sq =
    vel_sq_A, so with g = (g0, 0, g2) and a direction in A, lo and hi only, A's eight results, lo_bar_dot and hi_bar_dot are
    integrals_hvp_ref.hvp_ld's with g = (g0, 0, g2, 0).  Measured: 2.0e-17 random, 7.6e-18 solved."""
    for name, sp in (("random", tr.random_states(N, 5)), ("solved", xr.solved_golden(N))):
        lo, hi = xr.windows(sp, K, 21)
        T_A = np.asarray(sp[6]) + np.asarray(sp[7])
        c, zero = np.full(N, 7.0), np.zeros(N)
        b = [c, c, c, zero, zero, zero, T_A + 1.0, np.ones(N)]
        # a window end exactly on A's knot is a tie: the second derivative is one-sided there (acc jumps across the knot) and the two rules
        # take different sides -- section 19's ends segment 0 at hi, section 20's at the knot and walks a piece of length zero.  Those
        # queries (the windows' column 1) count with g = 0 in both
        d0 = np.asarray(sp[6])[:, None]
        tie = (lo == d0) | (hi == d0)
        assert 0 < tie.mean() < 0.2
        g = [np.where(tie, 0.0, x) for x in hr.gradients(lo.shape, 61)]
        dots, lo_dot, hi_dot = ih.directions(sp, lo, 62)
        ours = hr.hvp_ld(sp, b, lo, hi, None, [g[0], None, g[2]], dots, None, lo_dot, hi_dot, None)
        theirs = ih.hvp_ld(sp, lo, hi, [g[0], None, g[2], None], dots, lo_dot, hi_dot)
        err = float(np.max(tr.normwise(list(ours[0]) + [ours[2], ours[3]], ih.flat(theirs))))
        print("%-7s against the single-spline integrals' HVP, normwise: %.2e" % (name, err))
        assert err <= 1e-12, (name, err)


def test_known_second_derivative():
    """A constant at 3 with durations (1, 1), B constant at 1 with durations (1, 1.5), delay 0, the whole domain: gap_sq = D^2 T_A with
    D = 2, the end is END_A.  Along +1 on A's three positions: A's three position results sum to 2 T_A = 4, B's to -4, and
    d2 / dp dT = 2 D = 4 on both of A's durations; B's durations get 0.  Derived by longdouble central differences first."""
    col = lambda *x: [np.array([v]) for v in x]      # noqa: E731
    a, b = col(3.0, 3.0, 3.0, 0.0, 0.0, 0.0, 1.0, 1.0), col(1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.5)
    g = [None, np.ones((1, 1)), None]
    shift = [np.ones(1)] * 3 + [np.zeros(1)] * 5
    e = 2.0 ** -20

    def summary(bars_a, bars_b):
        return [float(sum(bars_a[:3])[0]), float(sum(bars_b[:3])[0]), float(bars_a[6][0]), float(bars_a[7][0]), float(bars_b[6][0]),
                float(bars_b[7][0])]

    up = kr.vjp_ld([x + e * d for x, d in zip(a, shift)], b, None, None, None, g)
    dn = kr.vjp_ld([x - e * d for x, d in zip(a, shift)], b, None, None, None, g)
    by_differences = summary([(x - y) / (2 * LD(e)) for x, y in zip(up[0], dn[0])], [(x - y) / (2 * LD(e)) for x, y in zip(up[1], dn[1])])
    want = [4.0, -4.0, 4.0, 4.0, 0.0, 0.0]
    assert np.allclose(by_differences, want, rtol=0, atol=1e-9), by_differences
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars_a, bars_b, _, _, _ = hvp(a, b, None, None, None, g, shift, None, None, None, None)
        got = summary(bars_a, bars_b)
        assert all(abs(x - y) <= 1e-13 * 4 for x, y in zip(got, want)), (hvp.__name__, got)


def test_float64_restatement_against_longdouble(families):
    """The kernel's arithmetic and order against the definition, normwise per problem, every query and every output: the device check's
    yardstick.  Measured worst: 5.2e-14 (random), 2.8e-15 solved, 2.9e-15 follower, 3.1e-15 follower0."""
    overall = 0.0
    for name, (a, b, lo, hi, delay) in families.items():
        g = hr.gradients(lo.shape, 51)
        d = hr.directions(a, b, lo, hi, delay, 52)
        worst = float(np.max(tr.normwise(hr.flat(hr.hvp_f64(a, b, lo, hi, delay, g, *d)), hr.flat(hr.hvp_ld(a, b, lo, hi, delay, g, *d)))))
        overall = max(overall, worst)
        print("%-9s float64 restatement of the HVP against longdouble, normwise: %.2e" % (name, worst))
        assert worst <= F64_BOUND, (name, worst)
    print("worst of all: %.2e (asserted: %.0e)" % (overall, F64_BOUND))


def test_nan_rule_of_the_restatements():
    a, b, lo, hi, delay = kr.family("random", 16, 4)
    g = [np.ones(lo.shape) for _ in range(3)]
    d = hr.directions(a, b, lo, hi, delay, 54)
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        clean = hr.flat(hvp(a, b, lo, hi, delay, g, *d))
        for side in range(2):
            for row, (f, bad) in enumerate(((6, 0.0), (7, -1.0), (6, np.inf), (7, np.nan))):
                pa, pb = [x.copy() for x in a], [x.copy() for x in b]
                (pb if side else pa)[f][row] = bad
                got = hr.flat(hvp(pa, pb, lo, hi, delay, g, *d))
                assert all(np.isnan(_f(x)[row]) for x in got[:16]), (hvp.__name__, side, row)
                assert all(np.all(_f(x)[row] == 0) for x in got[16:]), (hvp.__name__, side, row)
                assert all(np.array_equal(np.delete(_f(x), row, axis=0), np.delete(_f(y), row, axis=0)) for x, y in zip(got, clean))
        # a query without an answer counts with gradients of zero: its own three results are 0, every other query's are as they were
        for at, bad in ((0, np.nan), (1, np.nan), (2, np.nan), (2, np.inf), (2, -np.inf)):
            q = [lo.copy(), hi.copy(), delay.copy()]
            q[at][3, 1] = bad
            got = hr.flat(hvp(a, b, *q, g, *d))
            assert all(x[3, 1] == 0 for x in got[16:]), (hvp.__name__, at, bad)
            assert all(np.array_equal(np.delete(_f(x).ravel(), 3 * 4 + 1), np.delete(_f(y).ravel(), 3 * 4 + 1)) for x, y in zip(got[16:], clean[16:]))
            assert all(np.array_equal(np.delete(_f(x), 3), np.delete(_f(y), 3)) and np.isfinite(_f(x)).all() for x, y in zip(got[:16], clean[:16]))
        # a NaN tangent on an end that is clamped is not read
        inf = np.full(lo.shape, np.inf)
        whole = hr.flat(hvp(a, b, -inf, inf, delay, g, *d[:2], None, None, d[4]))
        nan = hr.flat(hvp(a, b, -inf, inf, delay, g, *d[:2], np.full(lo.shape, np.nan), np.full(lo.shape, np.nan), d[4]))
        assert all(np.array_equal(_f(x), _f(y)) for x, y in zip(whole, nan)), hvp.__name__
