"""The position and velocity extremes without a GPU (rp_trajectory_extrema, rp_batch_extrema_device, trajectory_extrema, min_time_extrema;
DESIGN.md section 15): the entries exist and refuse bad arguments before any device call, the torch layer checks its arguments, and the
restatements of tests/extrema_ref.py -- the definition in longdouble, the kernel's rule in float64, the routing of the derivatives --
agree with a dense grid of the evaluator's definition, with each other and with central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

import crossing_ref as cr
import extrema_ref as xr
import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ENTRIES = ("rp_trajectory_extrema", "rp_batch_extrema_device")


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    text = header[header.index("how far and how fast at most"):]
    for word in ("onedpath_ip.cpp:1065-1088", "Windows", "Candidates", "the knot", "strict comparison", "Returned time bits", "envelope",
                 "(pos_min, pos_max, vel_min, vel_max)"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # entries only: the revision stays
    assert rp.trajectory_extrema.__name__ == "trajectory_extrema" and rp.min_time_extrema.__name__ == "min_time_extrema"
    assert callable(rp.Batch.extrema_device) and callable(capi.trajectory_extrema)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    four = capi.extrema_table
    all4, none4 = four([good] * 4), four([0] * 4)
    vp = ctypes.c_void_p
    ext, bad = lib.rp_trajectory_extrema, capi.RP_ERR_INVALID
    assert ext(0, None, 0, 4, table, vp(good), vp(good), all4, all4) == bad and b"positive" in lib.rp_last_error()
    assert ext(0, None, 4, 0, table, vp(good), vp(good), all4, all4) == bad
    assert ext(0, None, 4, 1 << 31, table, vp(good), vp(good), all4, all4) == bad and b"2^31" in lib.rp_last_error()
    assert ext(0, None, 4, 4, None, vp(good), vp(good), all4, all4) == bad
    assert ext(-1, None, 4, 4, table, vp(good), vp(good), all4, all4) == bad
    for f in range(8):      # the end velocities alone may be NULL: those calls fail later, for want of an output
        entries = [good] * 8
        entries[f] = 0
        assert ext(0, None, 4, 4, capi.pointer_table(entries), None, None, none4, none4) == bad
        assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), f
    # all eight outputs NULL, or both tables; a NULL window end is allowed and gets as far as this
    assert ext(0, None, 4, 4, table, None, None, none4, none4) == bad and b"no output" in lib.rp_last_error()
    assert ext(0, None, 4, 4, table, vp(good), vp(good), None, None) == bad and b"no output" in lib.rp_last_error()
    assert ext(0, None, 4, 4, table, vp(good), vp(good), none4, None) == bad and b"no output" in lib.rp_last_error()
    assert ext(0, None, 4, 4, table, vp(odd), vp(good), all4, all4) == bad and b"16-byte" in lib.rp_last_error()
    assert ext(0, None, 4, 4, table, vp(good), vp(odd), all4, all4) == bad and b"16-byte" in lib.rp_last_error()
    for f in range(4):
        one = [good] * 4
        one[f] = odd
        assert ext(0, None, 4, 4, table, None, None, four(one), None) == bad and b"16-byte" in lib.rp_last_error()
        assert ext(0, None, 4, 4, table, None, None, all4, four(one)) == bad and b"16-byte" in lib.rp_last_error()
    assert lib.rp_batch_extrema_device(None, vp(good), vp(good), 4, all4, all4) == bad
    with pytest.raises(rp.RpError):
        capi.trajectory_extrema(0, 0, 4, 4, [good] * 8, good, good)
    with pytest.raises(ValueError, match="four"):
        capi.extrema_table([good] * 3)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_extrema(x, x, x, x, x, x, win, win)                              # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_extrema(x, x, x, win, win)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_extrema([0.0] * 4, x, x, x, x, x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.min_time_extrema(np.zeros(4), x, x)
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
    real_check, real_apply, real_solve = autograd._check_is_tensor, autograd._TrajectoryExtrema.apply, autograd.min_time_solve
    autograd._check_is_tensor = lambda name, t, who: None
    autograd._TrajectoryExtrema.apply = lambda *a: stopped.append(a) or tuple(range(8))
    autograd.min_time_solve = lambda *a, **kw: stopped.append("solve") or (a[0],) * 5
    try:
        v, m = OnDevice(meta(4)), OnDevice(meta(4, 3))
        args = [v, v, v, v, v, v]
        with pytest.raises(TypeError, match="float64"):
            rp.trajectory_extrema(OnDevice(meta(4, dtype=torch.float32)), v, v, v, v, v, m, m)
        with pytest.raises(ValueError, match="lengths differ"):
            rp.trajectory_extrema(v, OnDevice(meta(5)), v, v, v, v, m, m)
        for wrong, kind, text in ((OnDevice(meta(5)), ValueError, "shape"), (OnDevice(meta(4, dtype=torch.float32)), TypeError, "float64"),
                                  (OnDevice(meta(4), torch.device("cuda", 1)), TypeError, "ROCm device")):
            for at in (3, 4, 5):
                bad = list(args)
                bad[at] = wrong
                with pytest.raises(kind, match=text):
                    rp.trajectory_extrema(*bad, m, m)
            with pytest.raises(kind, match=text):
                rp.trajectory_extrema(*args, vel2=wrong)
        for wrong, kind in ((OnDevice(meta(3, 3)), ValueError), (OnDevice(meta(4, 0)), ValueError), (OnDevice(meta(0)), ValueError),
                            (OnDevice(meta(4, 3, 2)), ValueError), (OnDevice(meta(4, 3, dtype=torch.float32)), TypeError),
                            (OnDevice(meta(4, 3), torch.device("cpu")), TypeError)):
            with pytest.raises(kind, match="lo"):
                rp.trajectory_extrema(*args, wrong, m)
            with pytest.raises(kind, match="hi"):
                rp.trajectory_extrema(*args, None, wrong)
            with pytest.raises(kind, match="min_time_extrema: hi"):      # before the solve: a bad window costs none
                rp.min_time_extrema(v, v, v, m, wrong)
        with pytest.raises(ValueError, match="lo has shape"):
            rp.trajectory_extrema(*args, m, OnDevice(meta(4, 2)))
        assert not stopped
        # good arguments reach the launch in the table's order, the window's ends last; None stays None
        assert rp.trajectory_extrema(*args, m, vel0=v) == tuple(range(8))
        assert len(stopped) == 1 and stopped[0][3] is v and stopped[0][4] is None and stopped[0][8] is m and stopped[0][9] is None
        assert rp.trajectory_extrema(*args)[7] == 7 and stopped[1][8] is None and stopped[1][9] is None
        out = rp.min_time_extrema(v, v, v, m, m)
        assert len(out) == 13 and out[:8] == tuple(range(8)) and stopped[2] == "solve" and len(stopped) == 4
    finally:
        autograd._check_is_tensor, autograd._TrajectoryExtrema.apply, autograd.min_time_solve = real_check, real_apply, real_solve


# ---------------------------------------------------------------- the restatements
N, K, GRID = 512, 8, 2001


@pytest.fixture(scope="module")
def families():
    """name -> (spline, lo, hi, the definition's (values, times), runner_up_gap): random unsolved states, the same with vel0 = vel2 = 0
    exactly, and the solved problems of tests/golden/f3_batch.npz."""
    out = {}
    for name, sp in (("random", tr.random_states(N, 5)), ("rest", cr.rest_to_rest(N, 6)), ("solved", xr.solved_golden(N))):
        lo, hi = xr.windows(sp, K, 21)
        out[name] = (sp, lo, hi, xr.extrema_ld(sp, lo, hi), xr.runner_up_gap(sp, lo, hi))
    return out


def _scale(sp, j):
    return tr.scales(sp)[0 if j < 2 else 1]


def test_windows_are_what_they_claim(families):
    for name, (sp, lo, hi, (values, _), _) in families.items():
        T = (sp[6] + sp[7])[:, None]
        assert np.all(np.isneginf(lo[:, 0])) and np.all(np.isposinf(hi[:, 0])) and np.all(lo[:, 1] == 0) and np.all(hi[:, 1] == sp[6]), name
        assert np.all(lo <= hi), name
        empty = (hi < 0) | (lo > T)
        assert 0.002 < empty[:, 2:].mean() < 0.03, (name, empty[:, 2:].mean())      # (0.1 / 1.2)^2 at either end: 1.4 %
        for v in values:
            assert np.array_equal(np.isnan(v), empty), name


def test_definition_against_a_dense_grid(families):
    """No point of a 2001-point grid over the clamped window beats the definition by more than 1e-13 x scale (what the grid misses it
    misses in the definition's favour), and each value is the evaluator's definition at the returned time, exactly."""
    worst = 0.0
    u = np.linspace(0.0, 1.0, GRID)[None, :].astype(LD)
    for name, (sp, lo, hi, (values, times), _) in families.items():
        T = (sp[6] + sp[7])[:, None]
        a, b = np.where(lo > 0, lo, 0.0), np.where(hi < T, hi, T)
        ok = a <= b
        for j in range(4):
            t = np.where(ok, times[j], LD(0))
            again = tr.forward_ld(sp, t)[0 if j < 2 else 1]
            assert np.array_equal(again[ok], values[j][ok]), (name, xr.NAMES[j])
            assert np.all((times[j] >= a)[ok] & (times[j] <= b)[ok]), (name, xr.NAMES[j])
        for col in range(K):
            aa, bb = np.where(ok[:, col], a[:, col], 0.0)[:, None].astype(LD), np.where(ok[:, col], b[:, col], 0.0)[:, None].astype(LD)
            pos, vel, _ = tr.forward_ld(sp, aa + u * (bb - aa))
            rows = ok[:, col]
            for j, (grid, sign) in enumerate(((pos, 1), (pos, -1), (vel, 1), (vel, -1))):
                best = (sign * grid).min(axis=1)      # the grid's minimum of sign * quantity
                beats = (sign * values[j][:, col] - best) / _scale(sp, j)[:, 0]
                worst = max(worst, float(np.max(beats[rows])))
    print("the grid exceeds the longdouble definition by at most %.2e of the scale" % worst)
    assert worst <= 1e-13


def test_float64_rule_against_the_definition(families):
    """The kernel's rule restated in float64 against the longdouble definition: the same NaN mask, values within 1e-13 x scale on every
    query (section 13's forward bound), times within 1e-12 T where the winner leads every candidate at another time by 1e-9 of the scale
    -- and the share of queries that comparison leaves out is capped."""
    worst_v = worst_t = 0.0
    for name, (sp, lo, hi, (values, times), gap) in families.items():
        v64, t64 = xr.extrema_f64(sp, lo, hi)
        T = (sp[6] + sp[7])[:, None]
        for j in range(4):
            ok = ~np.isnan(values[j])
            assert np.array_equal(np.isnan(v64[j]), ~ok) and np.array_equal(np.isnan(t64[j]), ~ok), (name, xr.NAMES[j])
            err = np.where(ok, np.abs(v64[j] - values[j]) / _scale(sp, j), 0)
            worst_v = max(worst_v, float(err.max()))
            assert np.array_equal(tr.forward_f64(sp, np.where(ok, t64[j], 0.0))[0 if j < 2 else 1][ok], v64[j][ok]), (name, xr.NAMES[j])
            clear = ok & (gap[j] >= 1e-9)
            worst_t = max(worst_t, float(np.where(clear, np.abs(t64[j] - times[j]) / T, 0).max()))
            # the share left out of the time comparison
            counted = ok.copy()
            cap = 0.01
            if name == "solved":
                cap = 0.05
                if xr.NAMES[j] == "vel_min":
                    counted[:, 0] = False      # vel(0) = vel(T) = 0 exactly: the whole spline's minimum velocity is a structural tie
            left = float((counted & ~clear).sum() / counted.sum())
            print("%s %s: %.2f %% of the queries left out of the time comparison" % (name, xr.NAMES[j], 100 * left))
            assert left <= cap, (name, xr.NAMES[j], left)
    print("float64 rule against the definition: values %.2e of the scale, times %.2e of T" % (worst_v, worst_t))
    assert worst_v <= 1e-13 and worst_t <= 1e-12


def test_the_knot_family_gives_the_knot_exactly():
    sp, lo, hi, kinds = xr.knot_cases()
    assert np.all(sp[5] == 0) and np.all((sp[1] > np.maximum(sp[0], sp[2])) | (sp[1] < np.minimum(sp[0], sp[2])))
    assert sorted(kinds) == sorted(xr.NAMES * 2)
    for f in (xr.extrema_ld, xr.extrema_f64):
        values, times = f(sp, lo, hi)
        for i, kind in enumerate(kinds):
            j = xr.NAMES.index(kind)
            want = sp[1][i] if j < 2 else sp[5][i]
            assert values[j][i, 0] == want and times[j][i, 0] == sp[6][i], (f.__name__, i, kind)
            assert xr.classes(sp, lo, hi, times[j])[i, 0] == xr.KNOT
    # acc changes sign across the knot in the velocity cases, vel in the position cases
    d0 = sp[6][:, None]
    before, after = tr.forward_ld(sp, d0 * (1 - 1e-9)), tr.forward_ld(sp, d0 * (1 + 1e-9))
    for i, kind in enumerate(kinds):
        q = 1 if kind.startswith("pos") else 2
        assert before[q][i, 0] * after[q][i, 0] < 0, (i, kind)
    # without the knot candidate the first case's maximum would be pos0 = pos2 = 0
    (times_p, valid_p, value_p), _ = xr.candidates_ld(sp, lo, hi)
    others = [v[0, 0] for c, (ok, v) in enumerate(zip(valid_p, value_p)) if ok[0, 0] and c != 3]
    assert max(others) == 0.0


def test_routing_against_central_differences(families):
    """derivative_ld against longdouble central differences of extrema_ld in all eight spline inputs and both window ends, step
    1e-6 max(|x|, 1), per output over the queries whose winner leads by 1e-2 of the scale, outside column 1: 1e-6 normwise, with at
    least half of the finite queries kept.  (Column 1's hi sits on the knot while duration0 is perturbed on its own: a genuine kink,
    difference quotients there miss by O(1).)"""
    worst = {}
    for name, (sp, lo, hi, (values, times), gap) in families.items():
        rng = np.random.default_rng(31)
        for j in range(4):
            finite = ~np.isnan(values[j])
            keep = finite & (gap[j] >= 1e-2)
            keep[:, 1] = False
            share = keep.sum() / finite[:, [0] + list(range(2, K))].sum()
            g = [np.zeros((N, K)) for _ in range(4)]
            g[j] = np.where(keep, rng.standard_normal((N, K)), 0.0)
            bars, lo_bar, hi_bar = xr.derivative_ld(sp, lo, hi, times, values, g)

            def F(spl, lo_, hi_):
                return np.where(keep, g[j] * xr.extrema_ld(spl, lo_, hi_)[0][j], LD(0))

            fd = []
            for f in range(8):
                h = LD(1e-6) * np.maximum(np.abs(sp[f]), 1.0).astype(LD)
                up, dn = [np.asarray(x, dtype=LD) for x in sp], [np.asarray(x, dtype=LD) for x in sp]
                up[f], dn[f] = up[f] + h, dn[f] - h
                fd.append(np.sum(F(up, lo, hi) - F(dn, lo, hi), axis=1) / (2 * h))
            ends = []
            for which, end in enumerate((lo, hi)):
                h = np.where(np.isfinite(end), 1e-6 * np.maximum(np.abs(end), 1.0), 1.0).astype(LD)      # an infinite end does not move
                e = end.astype(LD)
                moved = (F(sp, e + h, hi) - F(sp, e - h, hi)) if which == 0 else (F(sp, lo, e + h) - F(sp, lo, e - h))
                ends.append(moved / (2 * h))
            assert all(np.isfinite(np.asarray(x, dtype=np.float64)).all() for x in fd + ends), (name, xr.NAMES[j])
            rows = keep.any(axis=1)
            err = float(np.max(tr.normwise([b[rows] for b in bars] + [lo_bar[rows], hi_bar[rows]], [x[rows] for x in fd] + [x[rows] for x in ends])))
            worst[(name, xr.NAMES[j])] = err
            print("%s %s: %.0f %% of the finite queries kept, routing against central differences %.2e normwise" % (name, xr.NAMES[j], 100 * share, err))
            assert share >= 0.5, (name, xr.NAMES[j], share)
            # a NaN value has gradient 0; forward mode is the transpose
            assert np.all(lo_bar[~finite] == 0) and np.all(hi_bar[~finite] == 0)
            dots = [rng.standard_normal(N) for _ in range(8)]
            lo_dot, hi_dot = rng.standard_normal((N, K)), rng.standard_normal((N, K))
            vdot = xr.derivative_jvp_ld(sp, lo, hi, times, values, dots, lo_dot, hi_dot)[j]
            assert np.array_equal(np.isnan(vdot), ~finite)
            left = np.sum(np.where(keep, g[j] * vdot, LD(0)), axis=1)
            terms = [b * d for b, d in zip(bars, dots)] + [np.sum(lo_bar * lo_dot, axis=1), np.sum(hi_bar * hi_dot, axis=1)]
            size = sum(np.abs(t) for t in terms) + np.sum(np.abs(np.where(keep, g[j] * vdot, LD(0))), axis=1)
            assert float(np.max(np.abs(left - sum(terms)) / np.maximum(size, 1e-300))) < 1e-15, (name, xr.NAMES[j])
    assert max(worst.values()) < 1e-6, worst


def test_column_one_routes_to_hi(families):
    """Column 1 is (0, duration0) exactly: a winner on its end is the knot's time and hi's at once, and the priority gives it to hi --
    the derivative of that value in hi is the evaluator's in the time, in duration0 the evaluator's at a fixed time."""
    for name, (sp, lo, hi, (values, times), _) in families.items():
        for j in range(4):
            cls = xr.classes(sp, lo, hi, times[j])[:, 1]
            at_end = np.asarray(times[j][:, 1] == sp[6])
            assert np.all(cls[at_end] == xr.HI) and not np.any(cls == xr.KNOT), (name, xr.NAMES[j])
            at_start = np.asarray(times[j][:, 1] == 0)
            assert np.all(cls[at_start] == xr.LO), (name, xr.NAMES[j])
            g = [np.zeros((N, K)) for _ in range(4)]
            g[j][:, 1] = 1.0
            bars, lo_bar, hi_bar = xr.derivative_ld(sp, lo, hi, times, values, g)
            t1 = np.asarray(times[j], dtype=LD)[:, 1:2]
            zero = np.zeros((N, 1), dtype=LD)
            plain, tau_bar = tr.vjp_ld(sp, t1, *((np.ones((N, 1)), zero) if j < 2 else (zero, np.ones((N, 1)))), zero)
            assert np.array_equal(hi_bar[at_end, 1], tau_bar[at_end, 0]) and np.array_equal(lo_bar[at_start, 1], tau_bar[at_start, 0])
            assert np.array_equal(bars[6], plain[6]) and np.array_equal(bars[7], plain[7]), (name, xr.NAMES[j])
        assert at_end.any() or name != "solved"


def test_nan_rule_of_the_restatements():
    sp = tr.random_states(8, 9)
    lo, hi = xr.windows(sp, 5, 2)
    sp[6][1], sp[7][2], sp[6][3] = 0.0, np.inf, -1.0
    T = sp[6] + sp[7]
    lo[4, 2], hi[5, 3] = np.nan, np.nan                     # a NaN end
    lo[6, 2], hi[6, 2] = -2.0, -1.0                         # wholly before the spline
    lo[7, 3], hi[7, 3] = 1.5 * T[7], np.inf                 # wholly after it
    lo[0, 2], hi[0, 2] = 0.25 * T[0], 0.25 * T[0]           # a = b: one point
    lo[0, 3], hi[0, 3] = np.inf, np.inf
    lo[0, 4], hi[0, 4] = T[0], np.inf                       # a = b = T
    for f in (xr.extrema_ld, xr.extrema_f64):
        values, times = f(sp, lo, hi)
        for x in values + times:
            bad = np.isnan(np.asarray(x, dtype=np.float64))
            assert bad[1:4].all() and bad[4, 2] and bad[5, 3] and bad[6, 2] and bad[7, 3] and bad[0, 3], f.__name__
            assert not bad[[0, 4, 5, 6, 7], 0].any() and not bad[0, 2] and not bad[0, 4], f.__name__
        assert all(t[0, 2] == lo[0, 2] for t in times) and all(t[0, 4] == T[0] for t in times)
        assert values[0][0, 2] == values[1][0, 2] and values[2][0, 4] == values[3][0, 4]
        # whole-spline windows: the time is +0.0 or T when an end wins, never -inf / +inf
        assert all(np.all((t[[0, 4, 5, 6, 7], 0] >= 0) & (t[[0, 4, 5, 6, 7], 0] <= T[[0, 4, 5, 6, 7]])) for t in times)
