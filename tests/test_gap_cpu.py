"""The extreme gap between two splines without a GPU (rp_trajectory_gap, trajectory_gap, min_time_gap): the entry
exists and refuses bad arguments before any device call, the torch layer checks its arguments, and the restatements of tests/gap_ref.py
-- the definition in longdouble, the kernel's rule in float64, the routing of the derivatives -- agree with a dense grid of the
evaluator's definition, with each other and with central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

import gap_ref as gr
import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+rp_trajectory_gap\s*\(", header)
    assert "rp_trajectory_gap" in capi.SIGNATURES and hasattr(lib, "rp_trajectory_gap")
    text = header[header.index("how close two splines get"):]
    for word in ("pos_A(t) - pos_B(t - delay)", "common domain", "k_A first among equals", "strictly inside", "strict comparison",
                 "Returned time bits", "envelope", "(gap_min, gap_max)", "no batch entry", "clamp(max(gap_min, -gap_max), min = 0)"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # an entry only: the revision stays
    assert rp.trajectory_gap.__name__ == "trajectory_gap" and rp.min_time_gap.__name__ == "min_time_gap"
    assert callable(capi.trajectory_gap) and callable(capi.gap_table)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    two = capi.gap_table
    all2, none2 = two([good] * 2), two([0] * 2)
    vp = ctypes.c_void_p
    gap, bad = lib.rp_trajectory_gap, capi.RP_ERR_INVALID
    g = vp(good)
    assert gap(0, None, 0, 4, table, table, g, g, g, all2, all2) == bad and b"positive" in lib.rp_last_error()
    assert gap(0, None, 4, 0, table, table, g, g, g, all2, all2) == bad
    assert gap(0, None, 4, 1 << 31, table, table, g, g, g, all2, all2) == bad and b"2^31" in lib.rp_last_error()
    assert gap(0, None, 4, 4, None, table, g, g, g, all2, all2) == bad and b"d_spline_a" in lib.rp_last_error()
    assert gap(0, None, 4, 4, table, None, g, g, g, all2, all2) == bad and b"d_spline_b" in lib.rp_last_error()
    assert gap(-1, None, 4, 4, table, table, g, g, g, all2, all2) == bad
    for f in range(8):      # the end velocities of either table alone may be NULL: those calls fail later, for want of an output
        entries = [good] * 8
        entries[f] = 0
        for tables in ((capi.pointer_table(entries), table), (table, capi.pointer_table(entries))):
            assert gap(0, None, 4, 4, *tables, None, None, None, none2, none2) == bad
            assert (b"no output" in lib.rp_last_error()) == (f in (3, 4)), f
    # all four outputs NULL, or both tables; NULL window ends and a NULL delay are allowed and get as far as this
    assert gap(0, None, 4, 4, table, table, None, None, None, none2, none2) == bad and b"no output" in lib.rp_last_error()
    assert gap(0, None, 4, 4, table, table, g, g, g, None, None) == bad and b"no output" in lib.rp_last_error()
    assert gap(0, None, 4, 4, table, table, g, g, g, none2, None) == bad and b"no output" in lib.rp_last_error()
    for at in range(3):
        ends = [g, g, g]
        ends[at] = vp(odd)
        assert gap(0, None, 4, 4, table, table, *ends, all2, all2) == bad and b"16-byte" in lib.rp_last_error()
    for f in range(2):
        one = [good] * 2
        one[f] = odd
        assert gap(0, None, 4, 4, table, table, None, None, None, two(one), None) == bad and b"16-byte" in lib.rp_last_error()
        assert gap(0, None, 4, 4, table, table, None, None, None, all2, two(one)) == bad and b"16-byte" in lib.rp_last_error()
    with pytest.raises(rp.RpError):
        capi.trajectory_gap(0, 0, 4, 4, [good] * 8, [good] * 8, good, good, good)
    with pytest.raises(ValueError, match="two"):
        capi.gap_table([good] * 3)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_gap([x] * 6, [x] * 6, win, win, win)                              # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_gap([x] * 3, [x] * 3, win)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_gap([[0.0] * 4] + [x] * 5, [x] * 6)
    with pytest.raises(TypeError, match="list or tuple"):
        rp.trajectory_gap(x, [x] * 6)
    with pytest.raises(ValueError, match="six"):
        rp.trajectory_gap([x] * 6, [x] * 7)
    with pytest.raises(TypeError, match="three tensors"):
        rp.min_time_gap([x] * 2, [x] * 3)
    with pytest.raises(TypeError, match="pair"):
        rp.min_time_gap([x] * 3, [x] * 3, vel_b=[x])
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
    real_check, real_apply, real_solve = autograd._check_is_tensor, autograd._TrajectoryGap.apply, autograd.min_time_solve
    autograd._check_is_tensor = lambda name, t, who: None
    autograd._TrajectoryGap.apply = lambda *a: stopped.append(a) or tuple(range(4))
    autograd.min_time_solve = lambda *a, **kw: stopped.append("solve") or (a[0],) * 5
    try:
        v, m = OnDevice(meta(4)), OnDevice(meta(4, 3))
        six = [v] * 6
        with pytest.raises(TypeError, match="float64"):
            rp.trajectory_gap([OnDevice(meta(4, dtype=torch.float32))] + six[1:], six, m)
        with pytest.raises(ValueError, match="lengths differ"):
            rp.trajectory_gap(six, [v, OnDevice(meta(5))] + six[2:], m)
        for wrong, kind, text in ((OnDevice(meta(5)), ValueError, "shape"), (OnDevice(meta(4, dtype=torch.float32)), TypeError, "float64"),
                                  (OnDevice(meta(4), torch.device("cuda", 1)), TypeError, "ROCm device")):
            for at in (3, 4, 5):
                bad = list(six)
                bad[at] = wrong
                with pytest.raises(kind, match=text):
                    rp.trajectory_gap(bad, six, m)
                with pytest.raises(kind, match="trajectory_gap: b"):
                    rp.trajectory_gap(six, bad, m)
            with pytest.raises(kind, match=text):
                rp.trajectory_gap(six, six + [None, wrong])
        # the two vehicles: one n, one device
        five, other = [OnDevice(meta(5))] * 6, [OnDevice(meta(4), torch.device("cuda", 1))] * 6
        with pytest.raises(ValueError, match="a holds 4 problems, b 5"):
            rp.trajectory_gap(six, five, m)
        with pytest.raises(TypeError, match="a's ROCm device"):
            rp.trajectory_gap(six, other, m)
        with pytest.raises(ValueError, match="a holds 4 problems, b 5"):
            rp.min_time_gap(six[:3], five[:3], m)
        for wrong, kind in ((OnDevice(meta(3, 3)), ValueError), (OnDevice(meta(4, 0)), ValueError), (OnDevice(meta(0)), ValueError),
                            (OnDevice(meta(4, 3, 2)), ValueError), (OnDevice(meta(4, 3, dtype=torch.float32)), TypeError),
                            (OnDevice(meta(4, 3), torch.device("cpu")), TypeError)):
            with pytest.raises(kind, match="lo"):
                rp.trajectory_gap(six, six, wrong, m, m)
            with pytest.raises(kind, match="hi"):
                rp.trajectory_gap(six, six, None, wrong)
            with pytest.raises(kind, match="delay"):
                rp.trajectory_gap(six, six, None, None, wrong)
            with pytest.raises(kind, match="min_time_gap: delay"):      # before the solves: a bad query costs none
                rp.min_time_gap(six[:3], six[:3], m, m, wrong)
        with pytest.raises(ValueError, match="lo has shape"):
            rp.trajectory_gap(six, six, m, None, OnDevice(meta(4, 2)))
        with pytest.raises(ValueError, match="hi has shape"):
            rp.trajectory_gap(six, six, None, m, OnDevice(meta(4, 2)))
        assert not stopped
        # good arguments reach the launch in the tables' order, A's then B's, the queries last; None stays None
        w = OnDevice(meta(4))
        assert rp.trajectory_gap(six, six + [w, None], m) == tuple(range(4))
        call = stopped[0]
        assert len(stopped) == 1 and len(call) == 19 and call[3] is None and call[4] is None and call[11] is w and call[12] is None
        assert call[16] is m and call[17] is None and call[18] is None
        assert rp.trajectory_gap(six, six)[3] == 3 and stopped[1][16:] == (None, None, None)
        out = rp.min_time_gap(six[:3], six[:3], None, None, m, vel_a=(w, None))
        assert len(out) == 6 and out[:4] == tuple(range(4)) and len(out[4]) == 5 and len(out[5]) == 5
        assert stopped[2] == "solve" and stopped[3] == "solve" and len(stopped) == 5
        assert stopped[4][3] is w and stopped[4][4] is None and stopped[4][11] is None and stopped[4][18] is m
    finally:
        autograd._check_is_tensor, autograd._TrajectoryGap.apply, autograd.min_time_solve = real_check, real_apply, real_solve


# ---------------------------------------------------------------- the restatements
N, K, GRID = 512, 8, 2001
# The share of the finite queries whose winner leads every candidate at another time by 1e-2 of the scale, measured on the longdouble
# restatement alone, per family and output (DESIGN.md section 18's table); the difference test must keep at least half of each.
KEPT_BY_THE_RESTATEMENT = {("random", "gap_min"): 0.51, ("random", "gap_max"): 0.49, ("solved", "gap_min"): 0.50, ("solved", "gap_max"): 0.50,
                           ("follower", "gap_min"): 0.44, ("follower", "gap_max"): 0.25}


@pytest.fixture(scope="module")
def families():
    """name -> (A, B, lo, hi, delay, the definition's (values, times), runner_up_gap): random unsolved pairs, solved pairs of
    tests/golden/f3_batch.npz, the solved A against itself 25 lower and later, and the same with no delay."""
    out = {}
    a, b = gr.random_pair(N)
    out["random"] = (a, b, gr.delays(a, b, K, 41))
    a, b = gr.solved_pair(N)
    out["solved"] = (a, b, gr.delays(a, b, K, 42))
    b = gr.follower(a)
    out["follower"] = (a, b, gr.delays(a, b, K, 43, follow=True))
    out["follower0"] = (a, b, np.zeros((N, K)))
    for name, (a, b, delay) in out.items():
        lo, hi = gr.windows(a, b, delay, 44)
        out[name] = (a, b, lo, hi, delay, gr.gap_ld(a, b, lo, hi, delay), gr.runner_up_gap(a, b, lo, hi, delay))
    return out


def test_queries_are_what_they_claim(families):
    for name, (a, b, lo, hi, delay, (values, _), _) in families.items():
        S, E = gr._domain(a, b, delay)[:2]
        assert np.all(np.isneginf(lo[:, :2])) and np.all(np.isposinf(hi[:, :2])) and np.all(lo <= hi) and np.all(S < E), name
        T = np.minimum(a[6] + a[7], b[6] + b[7])[:, None]
        if name in ("random", "solved"):
            assert np.all(delay[:, [0, 2]] == 0) and np.all(np.abs(delay) <= 0.3 * T) and (delay < 0).mean() > 0.3 and (delay > 0).mean() > 0.3
        elif name == "follower":
            assert np.all((delay >= 0.02 * T) & (delay <= 0.3 * T)), name
        else:
            assert np.all(delay == 0), name
        empty = (hi < S) | (lo > E)
        assert 0.002 < empty[:, 2:].mean() < 0.03, (name, empty[:, 2:].mean())      # (0.1 / 1.2)^2 at either end: 1.4 %
        for v in values:
            assert np.array_equal(np.isnan(v), empty), name


def test_definition_against_a_dense_grid(families):
    """No point of a 2001-point grid over the clamped window beats the definition by more than 1e-13 x scale (what the grid misses it
    misses in the definition's favour), and each value is the difference of the evaluator's definition at the returned time, exactly."""
    worst = 0.0
    u = np.linspace(0.0, 1.0, GRID)[None, :].astype(LD)
    for name, (a, b, lo, hi, delay, (values, times), _) in families.items():
        S, E = gr._domain(a, b, delay)[:2]
        wa, wb = np.where(lo > S, lo, S), np.where(hi < E, hi, E)
        ok = wa <= wb
        sc = gr.scale(a, b)[:, 0]
        for j in range(2):
            t = np.where(ok, times[j], LD(0))
            again = tr.forward_ld(a, t)[0] - tr.forward_ld(b, t - delay.astype(LD))[0]
            assert np.array_equal(again[ok], values[j][ok]), (name, gr.NAMES[j])
            assert np.all((times[j] >= wa)[ok] & (times[j] <= wb)[ok]), (name, gr.NAMES[j])
        for col in range(K):
            rows = ok[:, col]
            aa, bb = np.where(rows, wa[:, col], 0.0)[:, None].astype(LD), np.where(rows, wb[:, col], 0.0)[:, None].astype(LD)
            grid_t = aa + u * (bb - aa)
            grid = tr.forward_ld(a, grid_t)[0] - tr.forward_ld(b, grid_t - delay[:, col:col + 1].astype(LD))[0]
            for j, sign in enumerate((1, -1)):
                beats = (sign * values[j][:, col] - (sign * grid).min(axis=1)) / sc
                worst = max(worst, float(np.max(beats[rows])))
    print("the grid exceeds the longdouble definition by at most %.2e of the scale" % worst)
    assert worst <= 1e-13


def test_float64_rule_against_the_definition(families):
    """The kernel's rule restated in float64 against the longdouble definition: the same NaN mask, values within 2e-13 x scale on every
    query (section 13's forward bound, twice: two evaluations are subtracted), times within 1e-12 max(T_A, T_B) where the winner leads
    every candidate at another time by 1e-9 of the scale -- and the share of queries that comparison leaves out is capped.  With no delay
    the follower's gap is the same 25 at every time: its values are held to the bound and its times are left out."""
    worst_v = worst_t = 0.0
    for name, (a, b, lo, hi, delay, (values, times), gap) in families.items():
        v64, t64 = gr.gap_f64(a, b, lo, hi, delay)
        T = np.maximum(a[6] + a[7], b[6] + b[7])[:, None]
        sc = gr.scale(a, b)
        for j in range(2):
            ok = ~np.isnan(values[j])
            assert np.array_equal(np.isnan(v64[j]), ~ok) and np.array_equal(np.isnan(t64[j]), ~ok), (name, gr.NAMES[j])
            worst_v = max(worst_v, float(np.where(ok, np.abs(v64[j] - values[j]) / sc, 0).max()))
            at = np.where(ok, t64[j], 0.0)
            again = tr.forward_f64(a, at)[0] - tr.forward_f64(b, at - delay)[0]
            assert np.array_equal(again[ok], v64[j][ok]), (name, gr.NAMES[j])
            if name == "follower0":
                assert float(np.where(ok, np.abs(v64[j] - 25.0) / sc, 0).max()) <= 2e-13 and float(np.abs(values[j][ok] - 25).max()) <= 2e-13 * sc.max()
                continue
            clear = ok & (gap[j] >= 1e-9)
            worst_t = max(worst_t, float(np.where(clear, np.abs(t64[j] - times[j]) / T, 0).max()))
            left = float((ok & ~clear).sum() / ok.sum())
            print("%s %s: %.2f %% of the queries left out of the time comparison" % (name, gr.NAMES[j], 100 * left))
            assert left <= (0.10 if name == "solved" else 0.01), (name, gr.NAMES[j], left)
    print("float64 rule against the definition: values %.2e of the scale, times %.2e of max(T_A, T_B)" % (worst_v, worst_t))
    assert worst_v <= 2e-13 and worst_t <= 1e-12


def test_the_knot_family_gives_its_candidates_exactly():
    a, b, lo, hi, delay, want = gr.knot_cases()
    assert sorted(w[3] for w in want) == sorted((gr.KNOT_A, gr.KNOT_B, gr.START, gr.END_B)) and delay[1, 0] != 0
    for f in (gr.gap_ld, gr.gap_f64):
        values, times = f(a, b, lo, hi, delay)
        for i, (j, value, time, cls) in enumerate(want):
            assert values[j][i, 0] == value and times[j][i, 0] == time, (f.__name__, i, float(values[j][i, 0]), float(times[j][i, 0]))
            assert gr.classes(a, b, lo, hi, delay, times[j])[i, 0] == cls, (f.__name__, i)
    # the times are the knots, the start and the end they are named after
    assert want[0][2] == a[6][0] and want[1][2] == delay[1, 0] + b[6][1] and want[2][2] == delay[2, 0]
    assert want[3][2] == delay[3, 0] + (b[6][3] + b[7][3]) and want[3][2] < a[6][3] + a[7][3]
    # in the two knot cases the relative velocity changes sign at the knot, and neither piece reports its root there
    times, valid, _ = gr.candidates_ld(a, b, lo, hi, delay)
    for i in (0, 1):
        t = np.array([[want[i][2]]], dtype=LD)
        one = lambda s: [x[i:i + 1] for x in s]      # noqa: E731
        rel = lambda at: float(tr.forward_ld(one(a), at)[1][0, 0] - tr.forward_ld(one(b), at - LD(delay[i, 0]))[1][0, 0])      # noqa: E731
        assert rel(t - LD(1e-6)) * rel(t + LD(1e-6)) < 0 and rel(t) == 0
        roots = [c for c in (1, 2, 4, 5, 7, 8) if valid[c][i, 0]]
        assert not roots, (i, roots)


def _difference_keep(name, delay, values, times, gap, j):
    """The queries of output j that the difference test keeps: a winner that leads by 1e-2 of the scale, and not the clamped start of a
    query whose delay is exactly 0 -- there the domain's start changes from the constant +0.0 to the delay itself as the delay is
    moved, a genuine kink: difference quotients across it give half the one-sided slope."""
    finite = ~np.isnan(values[j])
    keep = finite & (gap[j] >= 1e-2)
    return finite, keep, keep & ~((delay == 0) & np.asarray(times[j] == 0))


def test_routing_against_central_differences(families):
    """derivative_ld against longdouble central differences of gap_ld in all sixteen spline inputs, both window ends and the delay, step
    1e-6 max(|x|, 1), per output over the queries whose winner leads by 1e-2 of the scale: 1e-6 normwise, with at least half of what the
    restatement alone keeps; and the duality of derivative_ld and derivative_jvp_ld."""
    worst = {}
    for name, (a, b, lo, hi, delay, (values, times), gap) in families.items():
        if name == "follower0":
            continue      # structurally constant: every candidate ties
        rng = np.random.default_rng(31)
        for j in range(2):
            finite, alone, keep = _difference_keep(name, delay, values, times, gap, j)
            share_alone, share = alone.sum() / finite.sum(), keep.sum() / finite.sum()
            g = [np.zeros((N, K)) for _ in range(2)]
            g[j] = np.where(keep, rng.standard_normal((N, K)), 0.0)
            bars_a, bars_b, lo_bar, hi_bar, delay_bar = gr.derivative_ld(a, b, lo, hi, delay, times, values, g)

            def F(sa, sb, lo_, hi_, dl_):
                return np.where(keep, g[j] * gr.gap_ld(sa, sb, lo_, hi_, dl_)[0][j], LD(0))

            fd = []
            for which in range(2):
                for f in range(8):
                    sp = (a, b)[which]
                    h = LD(1e-6) * np.maximum(np.abs(sp[f]), 1.0).astype(LD)
                    up, dn = [np.asarray(x, dtype=LD) for x in sp], [np.asarray(x, dtype=LD) for x in sp]
                    up[f], dn[f] = up[f] + h, dn[f] - h
                    moved = F(up, b, lo, hi, delay) - F(dn, b, lo, hi, delay) if which == 0 else F(a, up, lo, hi, delay) - F(a, dn, lo, hi, delay)
                    fd.append(np.sum(moved, axis=1) / (2 * h))
            ends = []
            for which, end in enumerate((lo, hi, delay)):
                h = np.where(np.isfinite(end), 1e-6 * np.maximum(np.abs(end), 1.0), 1.0).astype(LD)      # an infinite end does not move
                e = end.astype(LD)
                args = [lo, hi, delay]
                args[which] = e + h
                up = F(a, b, *args)
                args[which] = e - h
                ends.append((up - F(a, b, *args)) / (2 * h))
            assert all(np.isfinite(np.asarray(x, dtype=np.float64)).all() for x in fd + ends), (name, gr.NAMES[j])
            rows = keep.any(axis=1)
            got = [x[rows] for x in bars_a + bars_b] + [lo_bar[rows], hi_bar[rows], delay_bar[rows]]
            err = float(np.max(tr.normwise(got, [x[rows] for x in fd] + [x[rows] for x in ends])))
            worst[(name, gr.NAMES[j])] = err
            print("%s %s: the restatement alone keeps %.1f %% of the finite queries, the test %.1f %%; routing against central differences %.2e normwise"
                  % (name, gr.NAMES[j], 100 * share_alone, 100 * share, err))
            assert share >= 0.5 * KEPT_BY_THE_RESTATEMENT[(name, gr.NAMES[j])], (name, gr.NAMES[j], share)
            assert abs(share_alone - KEPT_BY_THE_RESTATEMENT[(name, gr.NAMES[j])]) <= 0.01, (name, gr.NAMES[j], share_alone)
            # a NaN value has gradient 0; forward mode is the transpose
            assert all(np.all(x[~finite] == 0) for x in (lo_bar, hi_bar, delay_bar))
            da, db = [rng.standard_normal(N) for _ in range(8)], [rng.standard_normal(N) for _ in range(8)]
            lo_dot, hi_dot, delay_dot = (rng.standard_normal((N, K)) for _ in range(3))
            vdot = gr.derivative_jvp_ld(a, b, lo, hi, delay, times, values, da, db, lo_dot, hi_dot, delay_dot)[j]
            assert np.array_equal(np.isnan(vdot), ~finite)
            left = np.where(keep, g[j] * vdot, LD(0))
            terms = [x * d for x, d in zip(bars_a + bars_b, da + db)]
            terms += [np.sum(x * d, axis=1) for x, d in ((lo_bar, lo_dot), (hi_bar, hi_dot), (delay_bar, delay_dot))]
            size = sum(np.abs(t) for t in terms) + np.sum(np.abs(left), axis=1)
            assert float(np.max(np.abs(np.sum(left, axis=1) - sum(terms)) / np.maximum(size, 1e-300))) < 1e-15, (name, gr.NAMES[j])
    assert max(worst.values()) < 1e-6, worst


def test_nan_rule_of_the_restatements():
    a, b = tr.random_states(10, 9), tr.random_states(10, 10)
    delay = gr.delays(a, b, 5, 3)
    lo, hi = gr.windows(a, b, delay, 2)
    lo[:, 2:], hi[:, 2:] = -np.inf, np.inf                  # whole domains, but for what follows
    a[6][1], b[7][2], a[6][3], b[6][8] = 0.0, np.inf, -1.0, np.nan
    S, E = gr._domain(a, b, delay)[:2]
    lo[4, 2], hi[5, 3] = np.nan, np.nan                     # a NaN end
    lo[6, 2], hi[6, 2] = S[6, 2] - 2.0, S[6, 2] - 1.0       # wholly before the common domain
    lo[7, 3], hi[7, 3] = E[7, 3] + 0.5, np.inf              # wholly after it
    delay[9, 1], delay[9, 2], delay[9, 3] = np.nan, np.inf, -np.inf
    lo[0, 2], hi[0, 2] = 0.5 * (S[0, 2] + E[0, 2]), 0.5 * (S[0, 2] + E[0, 2])      # a = b: one point
    lo[0, 3], hi[0, 3] = np.inf, np.inf
    lo[0, 4], hi[0, 4] = E[0, 4], np.inf                    # a = b = E
    for f in (gr.gap_ld, gr.gap_f64):
        values, times = f(a, b, lo, hi, delay)
        for x in values + times:
            bad = np.isnan(np.asarray(x, dtype=np.float64))
            assert bad[[1, 2, 3, 8]].all() and bad[4, 2] and bad[5, 3] and bad[6, 2] and bad[7, 3] and bad[0, 3] and bad[9, 1:4].all(), f.__name__
            assert not bad[[0, 4, 5, 6, 7, 9], 0].any() and not bad[0, 2] and not bad[0, 4] and not bad[9, 4], f.__name__
        assert all(t[0, 2] == lo[0, 2] for t in times) and all(t[0, 4] == E[0, 4] for t in times)
        assert values[0][0, 2] == values[1][0, 2] and values[0][0, 4] == values[1][0, 4]
        # whole-domain queries: the time is S or E when an end wins, never -inf / +inf
        rows = [0, 4, 5, 6, 7, 9]
        assert all(np.all((t[rows, 0] >= S[rows, 0]) & (t[rows, 0] <= E[rows, 0])) for t in times)
