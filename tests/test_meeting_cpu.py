"""The meeting times of two splines without a GPU (rp_trajectory_meeting, trajectory_meeting, min_time_meeting): the
entry exists and refuses bad arguments before any device call, the torch layer checks its arguments, and the restatements of
tests/meeting_ref.py -- the definition in longdouble, the kernel's rule in float64, the implicit derivative -- agree with the gap they
invert, with each other, with the crossing of one spline and with central differences."""
import ctypes
import os
import re

import numpy as np
import pytest

import crossing_ref as cr
import gap_ref as gr
import meeting_ref as mr
import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS = mr.EPS
N, K, GRID = 512, 8, 2001
FAMILIES = ("random", "solved", "follower")
# The share of the reached queries that pass meeting_ref.difference_is_a_yardstick, measured on the longdouble restatement alone
# (DESIGN.md section 22's table); the difference test must keep at least half of each.
KEPT_BY_THE_RESTATEMENT = {"random": 0.94, "solved": 0.88, "follower": 0.87}
# Two longdouble meeting times of one event differ by the rounding of D, a few 1e-19 of the scale, over the closing velocity: 1e-17 of the
# scale once weighted by |relvel| (the residual's bound).  The same differences as plain times, in units of Tmax: the issue's 1e-17 holds
# where the closing velocity is of the order scale / Tmax and not on a sub-piece that moves D by 1e-6 of the scale; what the restatement
# measures against itself (swap 2.9e-16, the crossing 3.1e-17, the moved window 6.1e-17), times ten, stands in its place.
PLAIN_TIME = {"swap": 2.9e-15, "crossing": 3.1e-16, "window": 6.1e-16}


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+rp_trajectory_meeting\s*\(", header)
    assert "rp_trajectory_meeting" in capi.SIGNATURES and hasattr(lib, "rp_trajectory_meeting")
    text = header[header.index("when two splines meet"):]
    for word in ("inverse of rp_trajectory_gap", "pos_A(t) - pos_B(t - delay)", "k_A first among equals", "NULL counts as 0", "earliest t in [a, b]",
                 "nine monotone sub-pieces", "computed once", "with its own bits", "rp_trajectory_crossing's search", "at most 64", "d_relvel",
                 "bit for bit", "no batch entry", "d_time not NULL"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # an entry only: the revision stays
    assert rp.trajectory_meeting.__name__ == "trajectory_meeting" and rp.min_time_meeting.__name__ == "min_time_meeting"
    assert callable(capi.trajectory_meeting)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    table = capi.pointer_table([good] * 8)
    vp = ctypes.c_void_p
    meet, bad = lib.rp_trajectory_meeting, capi.RP_ERR_INVALID
    g = vp(good)
    assert meet(0, None, 0, 4, table, table, g, g, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
    assert meet(0, None, 4, 0, table, table, g, g, g, g, g, g) == bad
    assert meet(0, None, 4, 1 << 31, table, table, g, g, g, g, g, g) == bad and b"2^31" in lib.rp_last_error()
    assert meet(0, None, 4, 4, None, table, g, g, g, g, g, g) == bad and b"d_spline_a" in lib.rp_last_error()
    assert meet(0, None, 4, 4, table, None, g, g, g, g, g, g) == bad and b"d_spline_b" in lib.rp_last_error()
    assert meet(-1, None, 4, 4, table, table, g, g, g, g, g, g) == bad
    for f in range(8):      # the end velocities of either table alone may be NULL: those calls fail later, for want of the times
        entries = [good] * 8
        entries[f] = 0
        for tables in ((capi.pointer_table(entries), table), (table, capi.pointer_table(entries))):
            assert meet(0, None, 4, 4, *tables, None, None, None, None, None, g) == bad
            assert (b"d_time is null" in lib.rp_last_error()) == (f in (3, 4)), f
    # the times cannot be left out; a NULL level, NULL window ends and a NULL delay are allowed and get as far as this
    assert meet(0, None, 4, 4, table, table, None, None, None, None, None, None) == bad and b"d_time is null" in lib.rp_last_error()
    assert meet(0, None, 4, 4, table, table, g, g, g, g, None, g) == bad and b"d_time is null" in lib.rp_last_error()
    for at in range(6):
        arrays = [g] * 6
        arrays[at] = vp(odd)
        assert meet(0, None, 4, 4, table, table, *arrays) == bad and b"16-byte" in lib.rp_last_error(), at
    with pytest.raises(rp.RpError):
        capi.trajectory_meeting(0, 0, 4, 4, [good] * 8, [good] * 8, good, good, good, good)      # no d_time


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x = torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_meeting([x] * 6, [x] * 6, win, win, win, win)                         # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_meeting([x] * 3, [x] * 3, win)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_meeting([[0.0] * 4] + [x] * 5, [x] * 6)
    with pytest.raises(TypeError, match="list or tuple"):
        rp.trajectory_meeting(x, [x] * 6)
    with pytest.raises(ValueError, match="six"):
        rp.trajectory_meeting([x] * 6, [x] * 7)
    with pytest.raises(TypeError, match="three tensors"):
        rp.min_time_meeting([x] * 2, [x] * 3)
    with pytest.raises(TypeError, match="pair"):
        rp.min_time_meeting([x] * 3, [x] * 3, vel_b=[x])
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
    real_check, real_apply, real_solve = autograd._check_is_tensor, autograd._TrajectoryMeeting.apply, autograd.min_time_solve
    autograd._check_is_tensor = lambda name, t, who: None
    autograd._TrajectoryMeeting.apply = lambda *a: stopped.append(a) or ("time", "relvel")
    autograd.min_time_solve = lambda *a, **kw: stopped.append("solve") or (a[0],) * 5
    try:
        v, m = OnDevice(meta(4)), OnDevice(meta(4, 3))
        six = [v] * 6
        with pytest.raises(TypeError, match="float64"):
            rp.trajectory_meeting([OnDevice(meta(4, dtype=torch.float32))] + six[1:], six, m)
        with pytest.raises(ValueError, match="trajectory_meeting: b"):
            rp.trajectory_meeting(six, six[:4] + [OnDevice(meta(5))] + six[5:], m)
        five, other = [OnDevice(meta(5))] * 6, [OnDevice(meta(4), torch.device("cuda", 1))] * 6
        with pytest.raises(ValueError, match="a holds 4 problems, b 5"):
            rp.trajectory_meeting(six, five, m)
        with pytest.raises(TypeError, match="a's ROCm device"):
            rp.trajectory_meeting(six, other, m)
        with pytest.raises(ValueError, match="a holds 4 problems, b 5"):
            rp.min_time_meeting(six[:3], five[:3], m)
        for wrong, kind in ((OnDevice(meta(3, 3)), ValueError), (OnDevice(meta(4, 0)), ValueError), (OnDevice(meta(0)), ValueError),
                            (OnDevice(meta(4, 3, 2)), ValueError), (OnDevice(meta(4, 3, dtype=torch.float32)), TypeError),
                            (OnDevice(meta(4, 3), torch.device("cpu")), TypeError)):
            for at, name in enumerate(("level", "lo", "hi", "delay")):
                args = [None] * 4
                args[at] = wrong
                with pytest.raises(kind, match=name):
                    rp.trajectory_meeting(six, six, *args)
                with pytest.raises(kind, match="min_time_meeting: " + name):      # before the solves: a bad query costs none
                    rp.min_time_meeting(six[:3], six[:3], *args)
        with pytest.raises(ValueError, match="level has shape"):
            rp.trajectory_meeting(six, six, m, None, None, OnDevice(meta(4, 2)))
        with pytest.raises(ValueError, match="lo has shape"):
            rp.trajectory_meeting(six, six, None, m, OnDevice(meta(4, 2)))
        assert not stopped
        # good arguments reach the launch in the tables' order, A's then B's, the queries last; None stays None; the times come back
        w = OnDevice(meta(4))
        assert rp.trajectory_meeting(six, six + [w, None], m) == "time"
        call = stopped[0]
        assert len(stopped) == 1 and len(call) == 20 and call[3] is None and call[4] is None and call[11] is w and call[12] is None
        assert call[16] is m and call[17:] == (None, None, None)
        assert rp.trajectory_meeting(six, six) == "time" and stopped[1][16:] == (None, None, None, None)
        out = rp.min_time_meeting(six[:3], six[:3], None, None, None, m, vel_a=(w, None))
        assert len(out) == 3 and out[0] == "time" and len(out[1]) == 5 and len(out[2]) == 5
        assert stopped[2] == "solve" and stopped[3] == "solve" and len(stopped) == 5
        assert stopped[4][3] is w and stopped[4][4] is None and stopped[4][11] is None and stopped[4][16] is None and stopped[4][19] is m
    finally:
        autograd._check_is_tensor, autograd._TrajectoryMeeting.apply, autograd.min_time_solve = real_check, real_apply, real_solve


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families():
    """name -> (A, B, level, lo, hi, delay, reached, the definition's (time, sub-piece, (lo, hi) of it))"""
    out = {}
    for name in FAMILIES:
        a, b, level, lo, hi, delay, reached, odd = mr.family(name, N, K)
        print("%s: %d of %d queries have no eligible sub-piece; %.1f %% are reached levels" % (name, odd, N * K, 100 * reached.mean()))
        out[name] = (a, b, level, lo, hi, delay, reached, mr.meeting_ld(a, b, level, lo, hi, delay))
    return out


def test_queries_are_what_they_claim(families):
    for name, (a, b, level, lo, hi, delay, reached, _) in families.items():
        S, E = gr._domain(a, b, delay)[:2]
        assert np.all(np.isneginf(lo[:, :2])) and np.all(np.isposinf(hi[:, :2])), name
        if name == "follower":
            assert np.all(delay > 0), name
        else:
            assert np.all(delay[:, [0, 2]] == 0) and (delay < 0).mean() > 0.3 and (delay > 0).mean() > 0.3, name
        empty = (hi < S) | (lo > E)
        assert 0.002 < empty[:, 2:].mean() < 0.03 and not reached[empty].any(), name
        assert 0.80 < reached.mean() < 0.88 and np.all(np.isfinite(level)), (name, reached.mean())


def test_definition_inverts_the_gap_and_is_the_first(families):
    """D(meeting) - level in longdouble is a rounding of the scale; the NaN mask is that of the unreached and empty queries; and on a
    2001-point grid of [a, time) D - level keeps one sign: nothing earlier."""
    worst = 0.0
    u = np.linspace(0.0, 1.0, GRID)[None, :-1].astype(LD)
    for name, (a, b, level, lo, hi, delay, reached, (time, m, (t_lo, t_hi))) in families.items():
        assert np.array_equal(np.isnan(time), ~reached) and np.array_equal(m < 0, ~reached), name
        S, E = gr._domain(a, b, delay)[:2]
        wa, wb = np.where(lo > S, lo, S), np.where(hi < E, hi, E)
        assert np.all(((time >= wa) & (time <= wb) & (time >= t_lo) & (time <= t_hi))[reached]), name
        at = np.where(reached, time, LD(0))
        worst = max(worst, float(np.max(np.where(reached, np.abs(mr.gap_ld(a, b, at, delay)[0] - level), 0) / gr.scale(a, b))))
        for col in range(K):
            rows = reached[:, col]
            start = np.where(rows, wa[:, col], 0.0)[:, None].astype(LD)
            grid_t = start + u * (at[:, col:col + 1] - start)
            g = mr.gap_ld(a, b, grid_t, delay[:, col:col + 1])[0] - level[:, col:col + 1]
            one_sign = np.all(g * g[:, :1] > 0, axis=1) | (at[:, col] == start[:, 0])
            assert one_sign[rows].all(), (name, col)
    print("longdouble: D(meeting) - level %.2e of the scale" % worst)
    assert worst <= 1e-17


def test_float64_rule_against_the_definition(families):
    """The kernel's rule restated in float64 against the longdouble definition: the same NaN masks, each time inside the definition's
    sub-piece to 4 eps Tmax, the residual within (c) = 2e-13 scale + 4 eps Tmax |relvel| -- section 13's forward bound twice, as in section
    18, plus section 14's 2-ulp stop --, the closing velocity within 2e-13 max(X / tmin, 1), and fewer than 64 trips."""
    worst = [0.0, 0.0, 0]
    for name, (a, b, level, lo, hi, delay, reached, (want, _, (t_lo, t_hi))) in families.items():
        time, relvel, trips = mr.meeting_f64(a, b, level, lo, hi, delay)
        assert np.array_equal(np.isnan(time), np.isnan(want)) and np.array_equal(np.isnan(relvel), np.isnan(time)), name
        ok = ~np.isnan(time)
        T = mr.tmax(a, b, delay)
        assert np.all(((time >= t_lo - 4 * EPS * T) & (time <= t_hi + 4 * EPS * T))[ok]), name
        at = np.where(ok, time, 0.0).astype(LD)
        d_ld, v_ld = mr.gap_ld(a, b, at, np.where(ok, delay, 0.0))
        ratio = np.abs(d_ld - level) / (2e-13 * gr.scale(a, b) + 4 * EPS * T * np.abs(v_ld))
        vel_scale = np.maximum(tr.scales(a)[1], tr.scales(b)[1])
        worst[0] = max(worst[0], float(np.max(ratio[ok])))
        worst[1] = max(worst[1], float(np.max((np.abs(relvel - v_ld) / vel_scale)[ok])))
        worst[2] = max(worst[2], int(trips.max()))
        assert trips[ok].min() >= 1, name      # no reached level of these families sits on a breakpoint
        groups = trips.reshape(-1, 64).max(axis=1)
        print("%s: mean trips %.2f over the reached queries, %.2f over all; most %d; the largest of 64 consecutive queries %.2f on average"
              % (name, trips[ok].mean(), trips.mean(), trips.max(), groups.mean()))
    print("float64 rule: residual %.3f of its bound, relvel %.2e of its scale, most trips %d" % tuple(worst))
    assert worst[0] <= 1.0 and worst[1] <= 2e-13 and worst[2] < cr.TRIPS


def test_hand_made_cases_give_their_breakpoints_exactly():
    a, b, level, lo, hi, delay, want = mr.hand_made()
    assert want[0, 0] == a[6][0] and want[1, 0] == delay[1, 0] + b[6][1] and delay[1, 0] == 0.25      # k_A; k_B
    assert want[2, 0] == delay[2, 0] and want[3, 0] == lo[3, 0] and want[4, 0] == lo[4, 0] and want[6, 0] == lo[6, 0]
    assert np.all(level[4:7] == 25) and level[7, 0] == 24 and np.all(delay[4:] == 0)
    for time in (mr.meeting_ld(a, b, level, lo, hi, delay)[0], mr.meeting_f64(a, b, level, lo, hi, delay)[0]):
        time = np.asarray(time, dtype=np.float64)
        assert np.array_equal(time[:7], want[:7]) and np.isnan(time[7, 0]), time[:, 0]
        assert not np.signbit(time[5, 0])      # the clamp +0.0


def test_swapping_the_splines_mirrors_the_meeting(families):
    """meeting(A, B, level, lo, hi, delay) - delay is meeting(B, A, -level, lo - delay, hi - delay, -delay): the same event on B's clock."""
    worst = np.zeros(2)
    for name, (a, b, level, lo, hi, delay, reached, (time, _, _)) in families.items():
        with np.errstate(all="ignore"):
            other = mr.meeting_ld(b, a, -level, lo - delay, hi - delay, -delay)[0]
        assert np.array_equal(np.isnan(other), np.isnan(time)), name
        diff = np.where(reached, np.abs((time - delay.astype(LD)) - other), 0)
        relvel = np.abs(mr.gap_ld(a, b, np.where(reached, time, LD(0)), delay)[1])
        worst = np.maximum(worst, [float((diff / mr.tmax(a, b, delay)).max()), float((diff * relvel / gr.scale(a, b)).max())])
    print("swap symmetry, longdouble: %.2e of Tmax; times |relvel| %.2e of the scale" % tuple(worst))
    assert worst[0] <= PLAIN_TIME["swap"] and worst[1] <= 1e-17


def test_a_standing_partner_reduces_the_meeting_to_the_crossing():
    """B standing still at 0 for as long as A drives, no delay, the whole domain: the meeting is crossing_ref.crossing_ld(A, level)."""
    worst = np.zeros(2)
    for seed in (5, 6):
        sp = tr.random_states(N, seed) if seed == 5 else cr.rest_to_rest(N, seed)
        lv = cr.levels(sp, K, seed + 10)
        want = cr.crossing_ld(sp, lv)[0]
        time = mr.meeting_ld(sp, mr.standing(sp), lv)[0]
        assert np.array_equal(np.isnan(time), np.isnan(want)) and 0.1 < np.isnan(want).mean() < 0.2
        ok = ~np.isnan(want)
        diff = np.where(ok, np.abs(time - want), 0)
        vel = np.abs(tr.forward_ld(sp, np.where(ok, want, LD(0)))[1])
        worst = np.maximum(worst, [float((diff / (sp[6] + sp[7])[:, None]).max()), float((diff * vel / tr.scales(sp)[0]).max())])
    print("meeting with a standing partner against the crossing, longdouble: %.2e of T; times |vel| %.2e of the scale" % tuple(worst))
    assert worst[0] <= PLAIN_TIME["crossing"] and worst[1] <= 1e-17


def test_derivative_against_central_differences(families):
    """derivative_ld against longdouble central differences of meeting_ld in all sixteen spline inputs, the level and the delay, step
    1e-6 max(|x|, 1), over the reached queries that pass difference_is_a_yardstick: 1e-6 normwise, with at least half of what the
    restatement alone keeps; the duality of derivative_ld and derivative_jvp_ld; an unreached level contributes exactly 0."""
    worst = {}
    for name, (a, b, level, lo, hi, delay, reached, (time, _, _)) in families.items():
        rng = np.random.default_rng(31)
        keep = reached & mr.difference_is_a_yardstick(a, b, level, delay, time)
        share = keep.sum() / reached.sum()
        g = np.where(keep, rng.standard_normal((N, K)), 0.0)
        bars_a, bars_b, level_bar, delay_bar = mr.derivative_ld(a, b, delay, time, g)
        steps_a, steps_b, level_step, delay_step = mr.difference_steps(a, b, level, delay)

        def F(sa, sb, lv, dl):
            return np.where(keep, g * mr.meeting_ld(sa, sb, lv, lo, hi, dl)[0], LD(0))

        fd, stable = [], np.ones(N, dtype=bool)
        for which, steps in enumerate((steps_a, steps_b)):
            for f in range(8):
                sp = (a, b)[which]
                h = steps[f].astype(LD)
                up, dn = [np.asarray(x, dtype=LD) for x in sp], [np.asarray(x, dtype=LD) for x in sp]
                up[f], dn[f] = up[f] + h, dn[f] - h
                fu, fdn = (F(up, b, level, delay), F(dn, b, level, delay)) if which == 0 else (F(a, up, level, delay), F(a, dn, level, delay))
                stable &= ~(np.isnan(fu).any(axis=1) | np.isnan(fdn).any(axis=1))      # a kept query lost its meeting under the step
                fd.append(np.sum(fu - fdn, axis=1) / (2 * h))
        fu, fdn = F(a, b, level.astype(LD) + level_step, delay), F(a, b, level.astype(LD) - level_step, delay)
        fd_level = (fu - fdn) / (2 * level_step.astype(LD))
        stable &= ~(np.isnan(fu).any(axis=1) | np.isnan(fdn).any(axis=1))
        fu, fdn = F(a, b, level, delay + delay_step), F(a, b, level, delay - delay_step)      # the moved delay is a float64 again
        fd_delay = (fu - fdn) / (((delay + delay_step) - (delay - delay_step)).astype(LD))
        stable &= ~(np.isnan(fu).any(axis=1) | np.isnan(fdn).any(axis=1))
        rows = keep.any(axis=1) & stable
        got = [x[rows] for x in bars_a + bars_b] + [level_bar[rows], delay_bar[rows]]
        err = float(np.max(tr.normwise(got, [x[rows] for x in fd] + [fd_level[rows], fd_delay[rows]])))
        worst[name] = err
        print("%s: the restatement keeps %.1f %% of the reached queries, %.1f %% of the problems stay; against central differences %.2e normwise"
              % (name, 100 * share, 100 * rows.mean(), err))
        assert share >= 0.5 * KEPT_BY_THE_RESTATEMENT[name] and abs(share - KEPT_BY_THE_RESTATEMENT[name]) <= 0.01, (name, share)
        assert rows.mean() > 0.9, name
        # an unreached level: exactly 0; forward mode is the transpose
        assert np.all(level_bar[~reached] == 0) and np.all(delay_bar[~reached] == 0), name
        da, db = [rng.standard_normal(N) for _ in range(8)], [rng.standard_normal(N) for _ in range(8)]
        level_dot, delay_dot = rng.standard_normal((N, K)), rng.standard_normal((N, K))
        tdot = mr.derivative_jvp_ld(a, b, delay, time, da, db, level_dot, delay_dot)
        assert np.array_equal(np.isnan(tdot), ~reached), name
        left = np.where(keep, g * tdot, LD(0))
        terms = [x * d for x, d in zip(bars_a + bars_b, da + db)] + [np.sum(x * d, axis=1) for x, d in ((level_bar, level_dot), (delay_bar, delay_dot))]
        size = sum(np.abs(t) for t in terms) + np.sum(np.abs(left), axis=1)
        assert float(np.max(np.abs(np.sum(left, axis=1) - sum(terms)) / np.maximum(size, 1e-300))) < 1e-15, name
    assert max(worst.values()) < 1e-6, worst


def test_the_window_only_chooses_the_branch(families):
    """lo moved later and hi moved, both short of the meeting: the time is unchanged -- it depends on them through the branch only."""
    worst = np.zeros(2)
    for name, (a, b, level, lo, hi, delay, reached, (time, _, _)) in families.items():
        S, E = gr._domain(a, b, delay)[:2]
        wa, wb = np.where(lo > S, lo, S), np.where(hi < E, hi, E)
        t = np.where(reached, np.asarray(time, dtype=np.float64), 0.0)
        lo2 = np.where(reached, wa + 0.5 * (t - wa), lo)
        hi2 = np.where(reached, t + 0.5 * (wb - t), hi)
        moved = mr.meeting_ld(a, b, level, lo2, hi2, delay)[0]
        assert np.array_equal(np.isnan(moved), ~reached) and (lo2 > wa)[reached].mean() > 0.9 and (hi2 < wb)[reached].mean() > 0.9, name
        diff = np.where(reached, np.abs(moved - time), 0)
        relvel = np.abs(mr.gap_ld(a, b, np.where(reached, time, LD(0)), delay)[1])
        worst = np.maximum(worst, [float((diff / mr.tmax(a, b, delay)).max()), float((diff * relvel / gr.scale(a, b)).max())])
    print("window moved inside the branch: the longdouble time moves by %.2e of Tmax; times |relvel| %.2e of the scale" % tuple(worst))
    assert worst[0] <= PLAIN_TIME["window"] and worst[1] <= 1e-17


def test_nan_rule_of_the_restatements():
    a, b = tr.random_states(10, 9), tr.random_states(10, 10)
    delay = gr.delays(a, b, 5, 3)
    lo, hi = np.full(delay.shape, -np.inf), np.full(delay.shape, np.inf)
    a[6][1], b[7][2], a[6][3], b[6][8] = 0.0, np.inf, -1.0, np.nan
    level = np.zeros(delay.shape)
    with np.errstate(all="ignore"):      # every query asks for a level its gap has: D at a time inside the domain
        S, E = gr._domain(a, b, delay)[:2]
        mid = 0.5 * (S + E)
        level[:] = tr.forward_f64(a, mid)[0] - tr.forward_f64(b, mid - delay)[0]
    lo[4, 2], hi[5, 3] = np.nan, np.nan                     # a NaN end
    lo[6, 2], hi[6, 2] = S[6, 2] - 2.0, S[6, 2] - 1.0       # wholly before the common domain
    lo[7, 3], hi[7, 3] = E[7, 3] + 0.5, np.inf              # wholly after it
    delay[9, 1], delay[9, 2], delay[9, 3] = np.nan, np.inf, -np.inf
    level[0, 1], level[0, 2], level[0, 3] = np.nan, np.inf, -np.inf
    for f in (mr.meeting_ld, mr.meeting_f64):
        out = f(a, b, level, lo, hi, delay)
        bad = np.isnan(np.asarray(out[0], dtype=np.float64))
        assert bad[[1, 2, 3, 8]].all() and bad[4, 2] and bad[5, 3] and bad[6, 2] and bad[7, 3] and bad[9, 1:4].all() and bad[0, 1:4].all(), f.__name__
        assert not bad[[0, 4, 5, 6, 7, 9], 0].any() and not bad[0, 4] and not bad[9, 4] and not bad[4, 3], f.__name__
    time, relvel, trips = mr.meeting_f64(a, b, level, lo, hi, delay)
    assert np.array_equal(np.isnan(relvel), np.isnan(time)) and trips.max() < cr.TRIPS and np.all(trips[np.isnan(time)] == 0)
