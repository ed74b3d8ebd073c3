"""The integrals' second derivative without a GPU (rp_trajectory_integrals_hvp, trajectory_integrals(order=2), min_time_integrals(order=2);
DESIGN.md section 19): the entry exists and refuses bad arguments before any device call, the torch layer refuses an order that is neither
1 nor 2 before it looks at a device, and the two restatements of tests/integrals_hvp_ref.py -- the definition in longdouble, the kernel's
arithmetic and order of additions in float64 -- agree with central differences of the first-order definition (integrals_ref.vjp_ld), with
the identities a second derivative must satisfy, with known answers of the routing, and with each other.  Families and windows are
tests/test_integrals_cpu.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

import crossing_ref as cr
import extrema_ref as xr
import integrals_hvp_ref as hr
import integrals_ref as ir
import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N, K = 512, 8
F64_BOUND = 1e-12      # normwise per problem: 10 x the worst the float64 restatement shows below (1.6e-14), rounded up to a power of ten


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    name = "rp_trajectory_integrals_hvp"
    assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header)
    assert header.index("RP_API int rp_trajectory_integrals_jvp") < header.index("RP_API int " + name) < header.index("RP_API int rp_batch_integrals_device")
    comment = header[:header.index("RP_API int %s(" % name)].rsplit("/*", 1)[1]
    for word in ("replaces", "held fixed", "symmetric", "rp_trajectory_integrals_jvp", "vel_dot(c) / |acc(c)|", "same bits", "no atomics"):
        assert word in comment, word
    assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.rp_abi_version() == 7      # a new entry only
    assert callable(capi.trajectory_integrals_hvp)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    none = capi.pointer_table([0] * 8)
    four = capi.integrals_table
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID

    def hv(n=4, k=4, sp=table, lo=vp(good), hi=vp(good), g=four([good] * 4), dots=table, ld=vp(good), hd=vp(good), bars=table, lb=vp(good),
           hb=vp(good), dev=0):
        return lib.rp_trajectory_integrals_hvp(dev, None, n, k, sp, lo, hi, g, dots, ld, hd, bars, lb, hb)

    assert hv(sp=None) == bad and b"d_spline" in lib.rp_last_error()
    assert hv(n=0) == bad and b"positive" in lib.rp_last_error()
    assert hv(k=0) == bad and b"positive" in lib.rp_last_error()
    assert hv(k=1 << 31) == bad and b"2^31" in lib.rp_last_error()
    assert hv(dev=-1) == bad
    for f in range(8):      # every required pointer: the spline's entries but the end velocities (a NULL window end is -inf / +inf)
        entries = [good] * 8
        entries[f] = 0
        st = hv(sp=capi.pointer_table(entries), lo=None, hi=None, g=None, dots=None, ld=None, hd=None, bars=none, lb=None, hb=None)
        assert st == bad
        assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), f
    # a misaligned n x k pointer, wherever it is
    for name in ("lo", "hi", "ld", "hd", "lb", "hb"):
        assert hv(**{name: vp(odd)}) == bad and b"16-byte" in lib.rp_last_error(), name
    for f in range(4):
        one = [good] * 4
        one[f] = odd
        assert hv(g=four(one)) == bad and b"16-byte" in lib.rp_last_error(), f
    # all outputs NULL: a table of NULLs, and no table
    assert hv(bars=none, lb=None, hb=None) == bad and b"no output" in lib.rp_last_error()
    assert hv(bars=None, lb=None, hb=None) == bad and b"no output" in lib.rp_last_error()
    with pytest.raises(rp.RpError):
        capi.trajectory_integrals_hvp(0, 0, 4, 4, [good] * 8, good, good, [good] * 4, [good] * 8)


def test_an_order_that_is_neither_1_nor_2_is_refused_before_the_device_checks():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"trajectory_integrals: order must be 1 or 2, got 3"):
        rp.trajectory_integrals(x, x, x, x, x, x, win, win, order=3)
    with pytest.raises(ValueError, match=r"min_time_integrals: order must be 1 or 2, got 0"):
        rp.min_time_integrals(x, x, x, win, win, order=0)
    for order in (1, 2):      # a valid order goes on to the device checks
        with pytest.raises(TypeError, match="ROCm device"):
            rp.trajectory_integrals(x, x, x, x, x, x, win, win, order=order)
        with pytest.raises(TypeError, match="ROCm device"):
            rp.min_time_integrals(x, x, x, win, win, order=order)


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families():
    """name -> (spline, lo, hi): tests/test_integrals_cpu.py's families and windows."""
    out = {}
    for name, sp in (("random", tr.random_states(N, 5)), ("rest", cr.rest_to_rest(N, 6)), ("solved", xr.solved_golden(N))):
        out[name] = (sp,) + tuple(xr.windows(sp, K, 21))
        out[name + "/short"] = (sp,) + tuple(ir.short_windows(sp, K, 22))
    sp, lo, hi, _ = xr.knot_cases()
    out["knot"] = (sp, lo, hi)
    return out


def test_longdouble_hvp_against_central_differences_of_the_vjp(families):
    """(vjp_ld(x + e d) - vjp_ld(x - e d)) / 2 e at e = 1e-6 along d = max(|x|, 1) x a standard normal in all ten inputs, over the queries
    integrals_ref.kept_for_differences keeps less those with a velocity root within 1e-3 T of a clamped window end or a near-double root
    inside the window (integrals_hvp_ref.kept_for_hvp_differences), normwise per problem.  Measured: 2.0e-8 random, 2.8e-8 rest, 3.8e-9
    solved (truncation); kept 59.3 %, 59.5 %, 59.8 % of the finite queries; 58 % of the random family's kept queries have a sign change of
    the velocity inside the window."""
    e = LD(1e-6)
    for name in ("random", "rest", "solved"):
        sp, lo, hi = families[name]
        keep, inside = hr.kept_for_hvp_differences(sp, lo, hi)
        finite = ~np.isnan(np.asarray(ir.integrals_ld(sp, lo, hi)[0], dtype=np.float64))
        share = keep.sum() / finite[:, [0] + list(range(2, K))].sum()      # column 1 is left out, as in section 16
        with_root = (inside & keep).sum() / keep.sum()
        rng = np.random.default_rng(41)
        g = [np.where(keep, rng.standard_normal(lo.shape), 0.0) for _ in range(4)]
        dots, lo_dot, hi_dot = hr.directions(sp, lo, 42, scaled=(lo, hi))
        lo_dot, hi_dot = np.where(keep, lo_dot, 0.0), np.where(keep, hi_dot, 0.0)
        got = hr.hvp_ld(sp, lo, hi, g, dots, lo_dot, hi_dot)

        def moved(sign):
            with np.errstate(all="ignore"):      # the infinite ends of column 0, which is not kept
                return ([np.asarray(a, dtype=LD) + sign * e * np.asarray(d, dtype=LD) for a, d in zip(sp, dots)],
                        lo.astype(LD) + sign * e * lo_dot.astype(LD), hi.astype(LD) + sign * e * hi_dot.astype(LD))

        up, dn = ir.vjp_ld(*moved(+1), g), ir.vjp_ld(*moved(-1), g)
        fd = [(a - b) / (2 * e) for a, b in zip(hr.flat(up), hr.flat(dn))]
        fd[8], fd[9] = np.where(keep, fd[8], LD(0)), np.where(keep, fd[9], LD(0))
        err = tr.normwise(hr.flat(got), fd)[keep.any(axis=1)]
        print("%-7s longdouble HVP against central differences of the longdouble VJP: worst %.2e normwise; %.1f %% of the finite queries kept, "
              "%.1f %% of them with a sign change of the velocity inside the window" % (name, err.max(), 100 * share, 100 * with_root))
        assert share >= 0.5 and err.max() <= 1e-6, (name, share, err.max())
        if name == "random":
            assert with_root > 0.25, with_root      # the root term is exercised


def test_symmetry(families):
    """u^T H[g] v = v^T H[g] u within 1e-15 of the sum of |terms|, in longdouble."""
    for name, (sp, lo, hi) in families.items():
        g = hr.gradients(lo.shape, 43)
        u, v = hr.directions(sp, lo, 44), hr.directions(sp, lo, 45)
        left, size_l = hr.bilinear(hr.hvp_ld(sp, lo, hi, g, *v), u)
        right, size_r = hr.bilinear(hr.hvp_ld(sp, lo, hi, g, *u), v)
        asym = float(np.max(np.abs(left - right) / (size_l + size_r)))
        print("%-13s symmetry %.2e of the sum of |terms|" % (name, asym))
        assert asym <= 1e-15, name


def test_exact_zeros(families):
    for name in ("random", "rest", "solved", "random/short"):
        sp, lo, hi = families[name]
        n = len(sp[0])
        g = hr.gradients(lo.shape, 46)
        v = hr.directions(sp, lo, 47)
        for hvp in (hr.hvp_ld, hr.hvp_f64):
            # the spline moved as a whole: vel and acc do not change, so nothing of vel_sq, acc_sq and the distance does
            result = hvp(sp, lo, hi, [None] + g[1:], hr.translation(n), None, None)
            assert all(np.all(np.asarray(x) == 0) for x in hr.flat(result)), (name, hvp.__name__)
            # pos_int's integrand moves with it: the end terms' derivative is g where an end is taken, and lands where the end came from
            bars, lo_bar_dot, hi_bar_dot = hvp(sp, lo, hi, [g[0], None, None, None], hr.translation(n), None, None)
            core = ir._core(sp, lo, hi, LD)
            on0, on1 = core["seg"][0]["on"], core["seg"][1]["on"]
            from_lo, from_hi = (on0 | core["from_a"]) & core["lo_taken"], ((on0 & ~core["knot_end"]) | on1) & core["hi_taken"]
            assert from_lo.mean() > 0.5 and from_hi.mean() > 0.5, name
            assert np.array_equal(np.asarray(lo_bar_dot, dtype=np.float64), np.where(from_lo, -g[0], 0.0)), (name, hvp.__name__)
            assert np.array_equal(np.asarray(hi_bar_dot, dtype=np.float64), np.where(from_hi, g[0], 0.0)), (name, hvp.__name__)
            assert all(np.all(np.asarray(bars[f]) == 0) for f in range(6)), (name, hvp.__name__)
            # no upstream gradient: no second derivative
            zero = np.zeros(lo.shape)
            for none in ([zero] * 4, None, [None] * 4):
                assert all(np.all(np.asarray(x) == 0) for x in hr.flat(hvp(sp, lo, hi, none, *v))), (name, hvp.__name__)


def test_none_is_zeros(families):
    sp, lo, hi = families["random"]
    rng = np.random.default_rng(48)
    g = [rng.standard_normal(lo.shape), None, rng.standard_normal(lo.shape), None]
    z = np.zeros(lo.shape)
    dots = [rng.standard_normal(N) if f % 2 else None for f in range(8)]
    full = [d if d is not None else np.zeros(N) for d in dots]
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        a = hvp(sp, lo, hi, g, dots, None, z)
        b = hvp(sp, lo, hi, [g[0], z, g[2], z], full, z, z)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(hr.flat(a), hr.flat(b))), hvp.__name__


def _direction(name, sp, lo, seed):
    """A random direction in all ten inputs; on the rest-to-rest families (rest, solved) one that keeps the end velocities."""
    dots, lo_dot, hi_dot = hr.directions(sp, lo, seed)
    return (dots if name.startswith("random") or name == "knot" else hr.keeps_the_end_velocities(dots)), lo_dot, hi_dot


def test_float64_restatement_against_longdouble(families):
    """The kernel's arithmetic and order against the definition, normwise per problem, every query and every output: the device check's
    yardstick.  The rest-to-rest families go along directions that keep the end velocities (integrals_hvp_ref.keeps_the_end_velocities:
    along the others the distance's second derivative is one-sided at the spline's own ends).  Measured worst: 1.6e-14 (rest), 6.4e-15
    random, 6.5e-15 solved, 7.8e-15 on the short windows, 1.3e-15 knot."""
    overall = 0.0
    for name, (sp, lo, hi) in families.items():
        g = hr.gradients(lo.shape, 51)
        d = _direction(name, sp, lo, 52)
        worst = float(np.max(tr.normwise(hr.flat(hr.hvp_f64(sp, lo, hi, g, *d)), hr.flat(hr.hvp_ld(sp, lo, hi, g, *d)))))
        overall = max(overall, worst)
        print("%-13s float64 restatement of the HVP against longdouble, normwise: %.2e" % (name, worst))
        assert worst <= F64_BOUND, (name, worst)
    print("worst of all: %.2e (asserted: %.0e)" % (overall, F64_BOUND))


def test_the_splines_own_ends_against_central_differences_of_the_vjp():
    """Windows clamped to the spline's ends -- the whole spline (the default call), (-inf, 0.6 T) and (0.3 T, +inf) -- on the rest-to-rest
    families, where the velocity at the clamped end is zero: both restatements against central differences of vjp_ld along a direction
    in the positions, vel1, both durations and the window's ends that keeps the end velocities (what min_time_integrals feeds: the solve's
    duration tangents are not zero), all four outputs, normwise per problem.  Measured 7.5e-9 (rest), 1.3e-9 (solved).  And a known
    answer: a monotone rest-to-rest spline travels |pos2 - pos0| whatever its durations, so the distance's second derivative along
    duration1 is 0."""
    e = LD(1e-6)
    for name, sp in (("rest", cr.rest_to_rest(N, 6)), ("solved", xr.solved_golden(N))):
        T = (sp[6] + sp[7])[:, None]
        inf = np.full((N, 1), np.inf)
        lo, hi = np.concatenate([-inf, -inf, 0.3 * T], axis=1), np.concatenate([inf, 0.6 * T, inf], axis=1)
        g = hr.gradients(lo.shape, 61)
        dots, lo_dot, hi_dot = hr.directions(sp, lo, 62, scaled=(lo, hi))
        dots = hr.keeps_the_end_velocities(dots)
        assert np.abs(dots[6]).min() > 0 and np.abs(dots[7]).min() > 0

        def moved(sign):
            with np.errstate(all="ignore"):      # the infinite ends
                return ([np.asarray(a, dtype=LD) + sign * e * np.asarray(d, dtype=LD) for a, d in zip(sp, dots)],
                        lo.astype(LD) + sign * e * lo_dot.astype(LD), hi.astype(LD) + sign * e * hi_dot.astype(LD))

        up, dn = ir.vjp_ld(*moved(+1), g), ir.vjp_ld(*moved(-1), g)
        fd = [(a - b) / (2 * e) for a, b in zip(hr.flat(up), hr.flat(dn))]
        for hvp in (hr.hvp_ld, hr.hvp_f64):
            err = float(np.max(tr.normwise(hr.flat(hvp(sp, lo, hi, g, dots, lo_dot, hi_dot)), fd)))
            print("%-7s %s at the spline's own ends against central differences of the longdouble VJP: worst %.2e normwise" % (name, hvp.__name__, err))
            assert err <= 1e-6, (name, hvp.__name__, err)
    sp = xr.solved_golden(N)
    monotone = np.sign(sp[1] - sp[0]) == np.sign(sp[2] - sp[1])
    assert monotone.mean() > 0.5
    along = [np.zeros(N) for _ in range(7)] + [np.ones(N)]
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars, _, _ = hvp(sp, None, None, [None, np.ones((N, 1)), None, None], along, None, None)
        first, _, _ = ir.vjp_ld(sp, None, None, [None, np.ones((N, 1)), None, None])
        size = max(float(np.abs(np.asarray(b, dtype=np.float64)[monotone]).max()) for b in first)
        worst = max(float(np.abs(np.asarray(b, dtype=np.float64)[monotone]).max()) for b in bars)
        print("the distance of a monotone rest-to-rest spline along duration1: %s at most %.2e (its first derivatives: up to %.2e)" % (hvp.__name__, worst, size))
        assert worst <= 1e-9 * max(size, 1.0), (hvp.__name__, worst)


def test_routing_exactly(families):
    rng = np.random.default_rng(53)
    for name in ("random", "rest", "solved"):
        sp = families[name][0]
        n = len(sp[0])
        g = [rng.standard_normal((n, 1)) for _ in range(4)]
        dots = [rng.standard_normal(n) for _ in range(8)]
        ld, hd = rng.standard_normal((n, 1)), rng.standard_normal((n, 1))
        for hvp, T in ((hr.hvp_ld, LD), (hr.hvp_f64, np.float64)):
            # the whole spline: both ends are clamps -- nothing reaches lo or hi, and their tangents reach nothing
            bars, lo_bar_dot, hi_bar_dot = hvp(sp, None, None, g, dots, None, None)
            assert np.all(lo_bar_dot == 0) and np.all(hi_bar_dot == 0), name
            inf = np.full((n, 1), np.inf)
            moved = hvp(sp, -inf, inf, g, dots, ld, hd)
            assert all(np.array_equal(x, y) for x, y in zip(hr.flat(moved), hr.flat((bars, lo_bar_dot, hi_bar_dot)))), name
            assert all(np.abs(np.asarray(b, dtype=np.float64)).min() > 0 for b in bars), name
            # a window inside segment 0 touches nothing of segment 1
            d0 = np.asarray(sp[6])[:, None]
            bars, lo_bar_dot, hi_bar_dot = hvp(sp, 0.2 * d0, 0.7 * d0, g, dots, ld, hd)
            assert all(np.all(bars[at] == 0) for at in (2, 4, 7)), name                          # pos2, vel2, duration1
            assert np.abs(lo_bar_dot).min() > 0 and np.abs(hi_bar_dot).min() > 0 and np.abs(bars[6]).min() > 0, name
            # a window inside segment 1: its ends are local times, so what goes to lo and hi leaves duration0 again
            T_ = d0 + np.asarray(sp[7])[:, None]
            a, b = d0 + 0.2 * (T_ - d0), d0 + 0.7 * (T_ - d0)
            bars, lo_bar_dot, hi_bar_dot = hvp(sp, a, b, g, dots, ld, hd)
            assert all(np.all(bars[at] == 0) for at in (0, 3)), name                             # pos0, vel0
            terms, _, _ = hr._terms(sp, a, b, g, dots, ld, hd, T)
            assert np.array_equal(terms[12][:, 0], -(lo_bar_dot + hi_bar_dot)[:, 0]) and np.all(terms[13] == 0), name


def test_known_second_derivative():
    """pos = 0, 100, 0, velocities 0, durations 1 (section 16's known answer: acc_sq = 240000 over the whole spline).  acc_sq scales with
    (pos1 - pos0)^2 + (pos2 - pos1)^2 at fixed durations: 12 dx^2 / h^3 per segment, so along pos1 its second derivative is 2 x 24 = 48
    -- and -24 in pos0 and in pos2."""
    sp = [np.array([x]) for x in (0.0, 100.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0)]
    one, zero = np.ones((1, 1)), np.zeros(1)
    direction = [zero, np.ones(1), zero, zero, zero, zero, zero, zero]
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars, _, _ = hvp(sp, None, None, [None, None, None, one], direction, None, None)
        for at, want in ((0, -24.0), (1, 48.0), (2, -24.0)):
            assert abs(float(bars[at][0]) - want) <= 1e-13 * 48, (hvp.__name__, at, float(bars[at][0]))


def test_nan_rule_of_the_restatements():
    sp = [a.copy() for a in tr.random_states(64, 9)]
    lo, hi = xr.windows(sp, 5, 10)
    g = [np.ones(lo.shape) for _ in range(4)]
    dots, lo_dot, hi_dot = hr.directions(sp, lo, 54)
    clean = hr.hvp_f64(sp, lo, hi, g, dots, lo_dot, hi_dot)
    sp[6][3], sp[7][20], sp[6][40], sp[7][63] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[50, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    bad = np.zeros(lo.shape, dtype=bool)
    bad[[3, 20, 40, 63]] = True
    bad[10, 0] = bad[50, 4] = bad[11, 3] = True
    bad |= np.isnan(ir.integrals_f64(sp, lo, hi)[0])
    good = np.ones(64, dtype=bool)
    good[[3, 20, 40, 63]] = False
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars, lo_bar_dot, hi_bar_dot = hvp(sp, lo, hi, g, dots, lo_dot, hi_dot)
        # a NaN output counts with gradients of zero; its problem's other queries and every other problem are as they were
        assert np.all(lo_bar_dot[bad] == 0) and np.all(hi_bar_dot[bad] == 0), hvp.__name__
        assert all(np.isfinite(np.asarray(b, dtype=np.float64)[good]).all() and np.isnan(np.asarray(b, dtype=np.float64)[~good]).all() for b in bars)
    bars, lo_bar_dot, hi_bar_dot = hr.hvp_f64(sp, lo, hi, g, dots, lo_dot, hi_dot)
    untouched = good.copy()
    untouched[[10, 50, 11]] = False
    assert all(np.array_equal(x[untouched], y[untouched]) for x, y in zip(hr.flat((bars, lo_bar_dot, hi_bar_dot)), hr.flat(clean)))
    # a NaN tangent on an end that is taken: its own query's lo_bar_dot and its problem's sums are NaN, no other query's outputs are
    sp = tr.random_states(8, 11)
    d0, T = sp[6][:, None], (sp[6] + sp[7])[:, None]
    lo, hi = np.concatenate([0.2 * d0, 0.3 * T], axis=1), np.concatenate([0.6 * d0, 0.9 * T], axis=1)
    dots, lo_dot, hi_dot = hr.directions(sp, lo, 55)
    lo_dot[5, 0] = np.nan
    for hvp in (hr.hvp_ld, hr.hvp_f64):
        bars, lo_bar_dot, hi_bar_dot = hvp(sp, lo, hi, [np.ones(lo.shape)] * 4, dots, lo_dot, hi_dot)
        nan = np.isnan(np.asarray(lo_bar_dot, dtype=np.float64))
        assert nan[5, 0] and nan.sum() == 1 and not np.isnan(np.asarray(hi_bar_dot, dtype=np.float64)).any(), hvp.__name__
        for f, b in enumerate(bars):      # the query lies in segment 0: pos2, vel2 and duration1 are not reached
            b = np.asarray(b, dtype=np.float64)
            assert np.isnan(b[5]) == (f not in (2, 4, 7)) and np.isfinite(np.delete(b, 5)).all(), (hvp.__name__, f)
