"""The first time two vehicles moving in d axes come within a distance, without a GPU (rp_trajectory_contact, trajectory_contact,
min_time_contact): the entry exists and refuses bad arguments before any device call, the torch layer checks its
arguments, and the restatements of tests/contact_ref.py -- the definition in longdouble, the kernel's rule in float64, the implicit-function
derivative -- agree with a grid of the squared distance, with each other, with the meeting of one axis (section 22), with exact hand-made
cases and with central differences; the kernel's query code compiled for the host gives the float64 restatement's bits."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

import contact_ref as cf
import meeting_ref as mr
import rocket_path_amd as rp
import separation_ref as sr
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N, K, GRID = 512, 8, 2001
FAMILIES = ("random", "solved", "follower")
DIMS = (1, 2, 3)
N_DIFF = 32      # the problems of each family that the central differences run on


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+rp_trajectory_contact\s*\(", header)
    assert "rp_trajectory_contact" in capi.SIGNATURES and hasattr(lib, "rp_trajectory_contact")
    text = header[header.index("first come within a distance"):]
    for word in ("d_level_sq", "SQUARED distance", "required", "never reached", "six", "computed once", "inclusive", "its own bits",
                 "d_rate", "bit for bit 2.0 times", "NaN exactly where the time is", "no batch entry", "before any device"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # an entry only: the revision stays
    for name in ("trajectory_contact", "min_time_contact"):
        assert getattr(rp, name).__name__ == name
    assert callable(capi.trajectory_contact)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    con, bad = lib.rp_trajectory_contact, capi.RP_ERR_INVALID
    g = vp(good)
    for d in (1, 2, 3):
        table = capi.axes_table([good] * (8 * d), d)
        assert con(0, None, 0, 4, d, table, table, g, g, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
        assert con(0, None, 4, 0, d, table, table, g, g, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
        assert con(0, None, 4, 1 << 31, d, table, table, g, g, g, g, g, g) == bad and b"2^31" in lib.rp_last_error()
        assert con(0, None, 4, 4, d, None, table, g, g, g, g, g, g) == bad and b"d_spline_a" in lib.rp_last_error()
        assert con(0, None, 4, 4, d, table, None, g, g, g, g, g, g) == bad and b"d_spline_b" in lib.rp_last_error()
        assert con(-1, None, 4, 4, d, table, table, g, g, g, g, g, g) == bad
        for f in range(8 * d):      # the end velocities of any axis may be NULL: those calls fail later, for want of a level
            entries = [good] * (8 * d)
            entries[f] = 0
            for tables in ((capi.axes_table(entries, d), table), (table, capi.axes_table(entries, d))):
                assert con(0, None, 4, 4, d, *tables, None, None, None, None, g, None) == bad
                assert (b"d_level_sq is null" in lib.rp_last_error()) == (f % 8 in (3, 4)), (d, f)
        # the level and the time are required; the window, the delay and the rate are not, and such a call gets as far as the alignment
        assert con(0, None, 4, 4, d, table, table, None, g, g, g, g, g) == bad and b"d_level_sq is null" in lib.rp_last_error()
        assert con(0, None, 4, 4, d, table, table, g, g, g, g, None, g) == bad and b"d_time is null" in lib.rp_last_error()
        assert con(0, None, 4, 4, d, table, table, vp(odd), None, None, None, g, None) == bad and b"16-byte" in lib.rp_last_error()
        for at in range(6):
            arrays = [g] * 6
            arrays[at] = vp(odd)
            assert con(0, None, 4, 4, d, table, table, *arrays) == bad and b"16-byte" in lib.rp_last_error(), (d, at)
    big = capi.axes_table([good] * 32, 4)
    for d in (0, 4, -1):      # before the tables are looked at
        assert con(0, None, 4, 4, d, big, big, g, g, g, g, g, g) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        with pytest.raises(ValueError):
            capi.trajectory_contact(0, 0, 4, 4, d, [good] * 8, [good] * 8, good, good, good, good, good, good)
    with pytest.raises(ValueError, match="16 entries"):
        capi.trajectory_contact(0, 0, 4, 4, 2, [good] * 8, [good] * 16, good, good, good, good, good)
    with pytest.raises(rp.RpError):
        capi.trajectory_contact(0, 0, 4, 4, 2, [good] * 16, [good] * 16, good, good, good, good)      # no time
    with pytest.raises(rp.RpError):
        capi.trajectory_contact(0, 0, 4, 4, 2, [good] * 16, [good] * 16, None, d_time=good)      # no level


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    x, y = torch.zeros((4, 2), dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    win = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="not both"):      # before anything else
        rp.trajectory_contact([x] * 6, [x] * 6, win, level_sq=win)
    with pytest.raises(TypeError, match="not neither"):
        rp.trajectory_contact([x] * 6, [x] * 6)
    with pytest.raises(TypeError, match="not both"):
        rp.min_time_contact([x] * 3, [x] * 3, win, level_sq=win)
    with pytest.raises(TypeError, match="not neither"):
        rp.min_time_contact([x] * 3, [x] * 3, lo=win)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_contact([x] * 6, [x] * 6, win, win, win, win)                         # CPU tensors
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_contact([y] * 6, [y] * 8, level_sq=win)
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_contact([x] * 3, [x] * 3, win)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.trajectory_contact([[0.0] * 4] + [x] * 5, [x] * 6, win)
    with pytest.raises(TypeError, match="list or tuple"):
        rp.trajectory_contact(x, [x] * 6, win)
    with pytest.raises(ValueError, match="six"):
        rp.trajectory_contact([x] * 6, [x] * 7, win)
    for wrong in (torch.zeros((4, 0), dtype=torch.float64), torch.zeros((4, 4), dtype=torch.float64), torch.zeros((4, 2, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match="axes|shape"):      # d = 0, d = 4, three dimensions
            rp.trajectory_contact([wrong] * 6, [wrong] * 6, win)
        with pytest.raises(ValueError, match="d in 1..3"):
            rp.min_time_contact([wrong] * 3, [wrong] * 3, win)
    with pytest.raises(ValueError, match="a has 2 axes, b 1"):
        rp.trajectory_contact([x] * 6, [y] * 6, win)
    with pytest.raises(TypeError, match="three tensors"):
        rp.min_time_contact([x] * 2, [x] * 3, win)
    with pytest.raises(ValueError, match="pos_a has shape"):
        rp.min_time_contact([x] * 3, [torch.zeros((4, 3), dtype=torch.float64)] * 3, win)
    with pytest.raises(ValueError, match="synchronize=True"):
        rp.min_time_contact([x] * 3, [x] * 3, win, vel_a=(x, x))
    with pytest.raises(ValueError, match="synchronize=True"):
        rp.min_time_contact([x] * 3, [x] * 3, level_sq=win, vel_b=(None, x))


# ---------------------------------------------------------------- the restatements
@pytest.fixture(scope="module")
def families():
    """(name, d) -> (A, B, level, lo, hi, delay, reached, odd, the definition's sub-pieces, contact_ld's result, contact_f64's)"""
    out = {}
    for name in FAMILIES:
        for d in DIMS:
            a, b, level, lo, hi, delay, reached, odd, sub = cf.family(name, N, K, d)
            out[name, d] = (a, b, level, lo, hi, delay, reached, odd, sub, cf.contact_ld(a, b, level, lo, hi, delay, subpieces=sub),
                            cf.contact_f64(a, b, level, lo, hi, delay))
    return out


def _bound_c(a, b, t, delay, missing):
    """(|f_ld(t) - level| is compared with) B(t) + 4 eps Tmax |rate_ld(t)| at the float64 times t, 0 where missing."""
    at, dl = np.where(missing, 0.0, t), np.where(missing, 0.0, delay)
    f_at, gaps = sr.f_ld(a, b, at, dl)
    return f_at, sr.value_bound(a, b, gaps) + 4 * cf.EPS * cf.tmax(a, b, delay) * np.abs(np.asarray(cf.rate_ld(a, b, at, dl), dtype=np.float64))


def test_levels_are_what_they_claim(families):
    for (name, d), (a, b, level, lo, hi, delay, reached, odd, sub, (t_ld, m, _), _) in families.items():
        found = ~np.isnan(np.asarray(t_ld, dtype=np.float64))
        assert np.array_equal(found, reached), (name, d)      # a level drawn inside a sub-piece is reached, one drawn beyond the window's f is not
        assert 0.80 < reached.mean() < 0.87 and odd < 0.02 * reached.size, (name, d, reached.mean(), odd)
        print("%s d = %d: %.1f %% of the levels reached; %d of %d queries without an eligible sub-piece" % (name, d, 100 * reached.mean(), odd, reached.size))


def test_definition_holds_its_own_checks(families):
    """f_ld at contact_ld's time is the level to 1e-17 of the positional scale^2, and on a 2,001-point grid of [a, t*) f - level keeps one
    sign: no earlier contact."""
    worst = 0.0
    u = np.linspace(0.0, 1.0, GRID, endpoint=False)[None, :].astype(LD)
    for (name, d), (a, b, level, lo, hi, delay, reached, _, sub, (t_ld, _, _), _) in families.items():
        sc2 = sr.scales(a, b)[1]
        missing = np.isnan(np.asarray(t_ld, dtype=np.float64))
        f_at = sr.f_ld(a, b, np.where(missing, LD(0), t_ld), np.where(missing, 0.0, delay))[0]
        worst = max(worst, float(np.where(missing, 0, np.abs(f_at - level) / sc2).max()))
        wa = sub[0][0]
        for col in range(K):
            gone = missing[:, col]
            start, stop = np.where(gone, LD(0), wa[:, col])[:, None], np.where(gone, LD(0), t_ld[:, col])[:, None]
            f = sr.f_ld(a, b, start + u * (stop - start), np.where(gone, 0.0, delay[:, col])[:, None])[0] - level[:, col:col + 1]
            # the first grid point is a itself, where f may be at the level (a contact at the window's start has an empty [a, t*))
            moved = (stop > start)[:, 0] & ~gone
            assert np.all((f[moved] > 0).all(axis=1) | (f[moved] < 0).all(axis=1)), (name, d, col)
    print("f_ld at the definition's time against the level: %.2e of the scale^2" % worst)
    assert worst <= 1e-17


def test_float64_rule_against_the_definition(families):
    """The same NaN mask on every query; every float64 time inside the definition's sub-piece +- 4 eps Tmax; the residual |f_ld(t) - level|
    within bound (c) = B(t) + 4 eps Tmax |rate_ld(t)|; every search below the fixed trip bound; the rate NaN exactly where the time is."""
    worst = 0.0
    for (name, d), (a, b, level, lo, hi, delay, reached, _, _, (t_ld, _, (t_lo, t_hi)), (time, rate, trips, deepest)) in families.items():
        missing = np.isnan(np.asarray(t_ld, dtype=np.float64))
        assert np.array_equal(np.isnan(time), missing) and np.array_equal(np.isnan(rate), missing), (name, d)
        slack = 4 * cf.EPS * cf.tmax(a, b, delay)
        outside = ~missing & ((time < np.asarray(t_lo, dtype=np.float64) - slack) | (time > np.asarray(t_hi, dtype=np.float64) + slack))
        assert not outside.any(), (name, d, int(outside.sum()))
        f_at, bound = _bound_c(a, b, time, delay, missing)
        share = float(np.where(missing, 0, np.abs(f_at - level) / bound).max())
        worst = max(worst, share)
        assert deepest.max() < sr.TRIPS, (name, d)
        print("%s d = %d: residual %.3f of bound (c); search trips per query: mean %.1f, most %d, the longest single search %d"
              % (name, d, share, trips.mean(), trips.max(), deepest.max()))
    assert worst <= 1.0


def test_follower_without_a_delay_is_never_reached():
    """follower0: f is structurally 625 d, so a level off it by more than B is NaN in both restatements and no contact search runs."""
    for d in DIMS:
        a, b, lo, hi, delay = sr.family("follower0", 64, K, d)
        B = float(np.max(sr.value_bound(a, b, [np.full((64, K), 25.0)] * d)))
        for off in (-2.0 * B - 1.0, 2.0 * B + 1.0, -1e4):
            level = np.full((64, K), 625.0 * d + off)
            assert np.isnan(np.asarray(cf.contact_ld(a, b, level, lo, hi, delay)[0], dtype=np.float64)).all(), (d, off)
            time, rate, _, _ = cf.contact_f64(a, b, level, lo, hi, delay)
            assert np.isnan(time).all() and np.isnan(rate).all(), (d, off)


def test_one_axis_against_the_meeting(families):
    """d = 1 in longdouble: with r = sqrt(level) in float64 and the level passed as the longdouble product r r, contact_ld is the earlier of
    meeting_ref.meeting_ld at the levels +r and -r: the same NaN mask, and the times apart by 1e-17 of the scale^2 once multiplied by
    |rate| (the plain difference is root-conditioned, section 22)."""
    worst = [0.0, 0.0]
    for name in FAMILIES:
        a, b, level, lo, hi, delay, _, _, sub = families[name, 1][:9]
        with np.errstate(all="ignore"):
            r = np.sqrt(np.where(level >= 0, level, np.nan))
        usable = ~np.isnan(r)
        r = np.where(usable, r, 1.0)
        t_c = cf.contact_ld(a, b, r.astype(LD) * r.astype(LD), lo, hi, delay, subpieces=sub)[0]
        t_p, t_m = mr.meeting_ld(a[0], b[0], r, lo, hi, delay)[0], mr.meeting_ld(a[0], b[0], -r, lo, hi, delay)[0]
        want = np.where(np.isnan(t_p), t_m, np.where(np.isnan(t_m), t_p, np.minimum(t_p, t_m)))
        gone = np.isnan(np.asarray(want, dtype=np.float64))
        assert np.array_equal(np.isnan(np.asarray(t_c, dtype=np.float64))[usable], gone[usable]), name
        both = usable & ~gone
        rate = cf.rate_ld(a, b, np.where(both, t_c, LD(0)), np.where(both, delay, 0.0))
        sc2 = sr.scales(a, b)[1]
        worst[0] = max(worst[0], float(np.where(both, np.abs(t_c - want) * np.abs(rate) / sc2, 0).max()))
        worst[1] = max(worst[1], float(np.where(both, np.abs(t_c - want) / cf.tmax(a, b, delay), 0).max()))
    print("d = 1 against the meeting of one axis: time difference x |rate| %.2e of the scale^2; the plain difference %.2e of Tmax (not asserted)"
          % tuple(worst))
    assert worst[0] <= 1e-17


def _both(a, b, level, lo, hi, delay):
    t_ld = np.asarray(cf.contact_ld(a, b, level, lo, hi, delay)[0], dtype=np.float64)
    time, rate, _, _ = cf.contact_f64(a, b, level, lo, hi, delay)
    return (("contact_ld", t_ld, None), ("contact_f64", time, rate))


def test_hand_made_cases_are_exact():
    a, b, lo, hi, delay, want = sr.hand_made()
    least = np.array([[w[0]] for w in want])
    starts = [0.0, delay[1, 0], delay[2, 0], 0.0]
    for who, time, rate in _both(a, b, least, lo, hi, delay):      # the level is each listed minimum: the touch, with the listed time's bits
        for i, (_, t, _, _) in enumerate(want):
            assert time[i, 0] == t and not np.signbit(time[i, 0]), (who, i, time[i, 0])
        assert want[0][1] == a[1][6][0] == 1.0 and want[1][1] == delay[1, 0] == 0.5 and want[2][1] == 2.0 and want[3][1] == 0.5
        if rate is not None:
            assert rate[0, 0] == 0.0 and rate[3, 0] == 0.0 and rate[1, 0] != 0.0 and rate[2, 0] != 0.0, rate
    for who, time, _ in _both(a, b, least - 1.0, lo, hi, delay):      # below the minimum: never
        assert np.isnan(time).all(), who
    wa = np.array([[s] for s in starts])
    at_start = np.asarray(sr.f_ld(a, b, wa, delay)[0], dtype=np.float64)
    assert np.array_equal(at_start.astype(LD), sr.f_ld(a, b, wa, delay)[0])      # exact in float64
    for who, time, _ in _both(a, b, at_start, lo, hi, delay):      # the level f(a): a's own bits
        assert np.array_equal(time.view(np.uint64), wa.view(np.uint64)), (who, time)
    inner = np.array([[9.0 + 34.25 ** 2], [0.0], [0.0], [985.5625]])
    for who, time, _ in _both(a, b, inner, lo, hi, delay):      # strictly inside the first piece of problems 0 and 3
        missing = np.isnan(time)
        f_at, bound = _bound_c(a, b, time, delay, missing)
        for i in (0, 3):
            assert abs(time[i, 0] - 0.25) <= 4 * cf.EPS * 3.5 and abs(f_at[i, 0] - inner[i, 0]) <= bound[i, 0], (who, i, time[i, 0])
        assert missing[1, 0] and missing[2, 0], who      # 0 is below both minima


def test_derivative_against_central_differences(families):
    """derivative_ld against longdouble central differences of contact_ld in all 16 d spline inputs, the level and the delay, step 1e-6
    max(|x|, 1), on the first 32 problems' reached queries that pass the yardstick mask: 1e-6 normwise, the mask keeping at least half;
    the duality of derivative_ld and derivative_jvp_ld within 1e-15 of the sum of the terms' sizes; an unreached level contributes
    exactly 0."""
    worst = {}
    rows = slice(0, N_DIFF)
    for (name, d), (a, b, level, lo, hi, delay, reached, _, _, (t_ld, _, _), _) in families.items():
        a, b = [[x[rows] for x in s] for s in a], [[x[rows] for x in s] for s in b]
        level, lo, hi, delay, reached, time = (x[rows] for x in (level, lo, hi, delay, reached, t_ld))
        rng = np.random.default_rng(37)
        found = ~np.isnan(np.asarray(time, dtype=np.float64))
        keep = found & cf.difference_is_a_yardstick(a, b, level, delay, time)
        share = keep.sum() / found.sum()
        g = np.where(keep, rng.standard_normal(keep.shape), 0.0)
        bars_a, bars_b, level_bar, delay_bar = cf.derivative_ld(a, b, delay, time, g)
        steps_a, steps_b, level_step, delay_step = cf.difference_steps(a, b, level, delay)
        stable = np.ones(len(lo), dtype=bool)

        def F(va, vb, lv, dl):
            nonlocal stable
            t = cf.contact_ld(va, vb, lv, lo, hi, dl)[0]
            stable &= ~(np.isnan(np.asarray(t, dtype=np.float64)) & keep).any(axis=1)      # a kept query lost its contact under the step
            return np.where(keep, g * t, LD(0))

        fd, got = [], []
        for which in range(2):
            for x in range(d):
                for f in range(8):
                    h = (steps_a, steps_b)[which][x][f].astype(LD)
                    up, dn = ([[np.asarray(v, dtype=LD) for v in s] for s in (a, b)[which]] for _ in range(2))
                    up[x][f], dn[x][f] = up[x][f] + h, dn[x][f] - h
                    diff = F(up, b, level, delay) - F(dn, b, level, delay) if which == 0 else F(a, up, level, delay) - F(a, dn, level, delay)
                    fd.append(diff.sum(axis=1) / (2 * h))
                    got.append((bars_a, bars_b)[which][x][f])
        up, dn = level + level_step, level - level_step
        fd.append((F(a, b, up, delay) - F(a, b, dn, delay)) / (up - dn).astype(LD))
        got.append(level_bar)
        up, dn = delay + delay_step, delay - delay_step
        fd.append((F(a, b, level, up) - F(a, b, level, dn)) / (up - dn).astype(LD))
        got.append(delay_bar)
        some = keep.any(axis=1) & stable
        err = float(np.max(tr.normwise([x[some] for x in got], [x[some] for x in fd])))
        worst[name, d] = err
        print("%s d = %d: the yardstick mask keeps %.1f %% of the reached queries, %.1f %% of the problems stay; against central differences %.2e normwise"
              % (name, d, 100 * share, 100 * some.mean(), err))
        assert share >= 0.5, (name, d, share)
        assert some.mean() > 0.5, (name, d)
        assert np.all(level_bar[~found] == 0) and np.all(delay_bar[~found] == 0), (name, d)
        assert all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for s in bars_a + bars_b for v in s), (name, d)
        # forward mode is the transpose
        n = len(lo)
        da = [[rng.standard_normal(n) for _ in range(8)] for _ in range(d)]
        db = [[rng.standard_normal(n) for _ in range(8)] for _ in range(d)]
        level_dot, delay_dot = rng.standard_normal(lo.shape), rng.standard_normal(lo.shape)
        tdot = cf.derivative_jvp_ld(a, b, delay, time, da, db, level_dot, delay_dot)
        assert np.array_equal(np.isnan(tdot), ~found), (name, d)
        left = np.where(keep, g * tdot, LD(0))
        terms = [bar * dot for bars, dots in ((bars_a, da), (bars_b, db)) for sb, sd in zip(bars, dots) for bar, dot in zip(sb, sd)]
        terms += [np.sum(level_bar * level_dot, axis=1), np.sum(delay_bar * delay_dot, axis=1)]
        size = sum(np.abs(t) for t in terms) + np.sum(np.abs(left), axis=1)
        assert float(np.max(np.abs(np.sum(left, axis=1) - sum(terms)) / np.maximum(size, 1e-300))) < 1e-15, (name, d)
    assert max(worst.values()) < 1e-6, worst


def test_nan_rule_of_the_restatements():
    """Durations 0, -1, inf and NaN in any one of the 2 d splines, NaN window ends, NaN and infinite delays and levels: NaN exactly there, and
    no search runs for those queries."""
    for d in DIMS:
        a, b = sr.vehicles("random", 12, d)
        delay = sr.delays(a, b, 5, 3)
        lo, hi = np.full(delay.shape, -np.inf), np.full(delay.shape, np.inf)
        level = cf.levels(a, b, lo, hi, delay, 5)[0]
        reached = ~np.isnan(cf.contact_f64(a, b, level, lo, hi, delay)[0])
        a[0][6][1], b[d - 1][7][2], a[d - 1][6][3], b[0][6][8] = 0.0, np.inf, -1.0, np.nan
        lo[4, 2], hi[5, 3] = np.nan, np.nan
        delay[9, 1], delay[9, 2], delay[9, 3] = np.nan, np.inf, -np.inf
        level[10, 0], level[10, 1], level[10, 2] = np.nan, np.inf, -np.inf
        spoilt = np.zeros(delay.shape, dtype=bool)
        spoilt[[1, 2, 3, 8]] = True
        spoilt[4, 2] = spoilt[5, 3] = True
        spoilt[9, 1:4] = spoilt[10, 0:3] = True
        t_ld = np.asarray(cf.contact_ld(a, b, level, lo, hi, delay)[0], dtype=np.float64)
        time, rate, trips, deepest = cf.contact_f64(a, b, level, lo, hi, delay)
        for who, x in (("contact_ld", t_ld), ("contact_f64", time), ("rate", rate)):
            assert np.isnan(x[spoilt]).all(), (who, d)
            assert np.array_equal(~np.isnan(x[~spoilt]), reached[~spoilt]), (who, d)
        assert np.all(trips[spoilt] == 0) and deepest.max() < sr.TRIPS and trips[~spoilt].max() > 0, d


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_kernel_source_on_the_host_gives_the_bits_of_the_restatement(capsys):
    """tests/checks/contact_host_cut.py: contact_query and its helpers cut out of csrc/trajectory.hip and csrc/spline_core.h, compiled into a
    stand-alone program with its own main under the address and undefined-behaviour sanitizers and run at 256 pairs on the random, solved
    and follower families, the follower without a delay and the NaN-rule inputs, d = 1, 2, 3: contact_f64's bits in every time, rate and
    trip count, every search ended, no sanitizer report.  Nothing is loaded into Python under a sanitizer."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "checks"))
    import contact_host_cut
    contact_host_cut.main(256)
    assert capsys.readouterr().out.count("time the same bits, rate the same bits, trips the same bits") == 15
