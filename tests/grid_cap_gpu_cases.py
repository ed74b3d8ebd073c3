"""The cases of tests/test_gpu_grid_cap.py, each run in a fresh process (`python tests/grid_cap_gpu_cases.py <case> [arguments]`), on top of
the helpers of every pair and fleet family.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why: DESIGN.md
section 30, "Beyond the grid's cap".  Every kernel written after section 13's grid cap, on launches of more trips than the grid has blocks
(trajectory_gpu_cases.GRID_N problems; fleets of m = 3 vehicles in 100,001 scenes, 300,003 pair-problems and as many vehicles), at k = 1 and
k = 7, where a block stages 128 problems per trip:

1. trajectory_gpu_cases.GRID_ROWS of every output -- for a fleet the scenes that hold those problems -- equal, bit for bit, the same rows
   run as a batch of their own;
2. no output element of the full launch is left at Out's sentinel, and the padding behind every output is intact;
3. the 385 rows around problem 262,144, where the blocks start their second trip, against the family's longdouble definition with the
   comparison, the tolerance and the cap on left-out queries of the family's own test_forward_against_the_definition;
4. a fleet form is bit for bit the pair entry on the gathered pairs, both at full size.

The splines, delays and windows are the families' own generators at these sizes.  The levels of the meeting and contact queries are the
families' own (meeting_ref.levels, contact_ref.levels: longdouble) on the rows of item 3; on the others, which items 1, 2 and 4 read, a
float64 stand-in (_plain_levels), since the longdouble generator on two million queries would take minutes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_cull_gpu_cases as fu  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402

import contact_gpu_cases as cg  # noqa: E402
import contact_ref as cf  # noqa: E402
import fleet_contact_gpu_cases as fc  # noqa: E402
import fleet_gpu_cases as fg  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import gap_ref as gr  # noqa: E402
import meeting_gpu_cases as mg  # noqa: E402
import meeting_ref as mr  # noqa: E402
import separation_gpu_cases as sg  # noqa: E402
import separation_ref as sr  # noqa: E402
import staggered_gpu_cases as st  # noqa: E402
import staggered_inputs as si  # noqa: E402
import tracking_gpu_cases as tk  # noqa: E402
import tracking_ref as kr  # noqa: E402
import trajectory_gpu_cases as tg  # noqa: E402
import trajectory_ref as tr  # noqa: E402

LD = np.longdouble
GRID_N, GRID_ROWS, SENTINEL = tg.GRID_N, tg.GRID_ROWS, tg.SENTINEL
MID = GRID_ROWS[1]
KS = (1, 7)      # the single trailing query; a thread's two queries in two problems and, in a fleet, in two scenes' window rows
M, SCENES = 3, 100001      # three pairs and three vehicles per scene: 300,003 problems for the pair kernels and for k_reach
PAIRS = M * (M - 1) // 2
# the scenes that hold GRID_ROWS' problems (and, M = PAIRS, the vehicles of those numbers): whole scenes, the last ones of the launch
FLEET_ROWS = tuple(slice(r.start // PAIRS, (r.stop - 1) // PAIRS + 1)
                   for r in (GRID_ROWS[0], MID, slice(SCENES * PAIRS - 257, SCENES * PAIRS)))
MID_SCENES = FLEET_ROWS[1]
_rows, _same_bits = tg._rows, tg._same_bits


def _kept(run):
    """(run, the outputs of its first call): rows_equal_their_own_batch makes the full launch first"""
    first = []

    def wrapped(*arrays):
        out = run(*arrays)
        if not first:
            first.append(out)
        return out
    return wrapped, first


def scenes_equal_their_own_batch(what, run, *arrays):
    """trajectory_gpu_cases.rows_equal_their_own_batch with the scene as the first axis and FLEET_ROWS; the full launch's outputs"""
    full = run(*arrays)
    for rows in FLEET_ROWS:
        own = run(*[_rows(a, rows) for a in arrays])
        assert len(own) == len(full)
        for j, (a, b) in enumerate(zip(full, own)):
            assert _same_bits(a[rows], b), (what, rows, "output %d" % j)
    return full


def _covered(full, what):
    """Every element of every output was written: none is left at the sentinel (Out.get has looked at the padding behind each)."""
    for j, x in enumerate(full):
        assert not np.any(x == SENTINEL), (what, "output %d" % j, "%d elements never written" % int((x == SENTINEL).sum()))


def _plain_levels(a, b, lo, hi, delay, seed, squared):
    """The stand-in levels of the rows nobody compares with a reference, (n, k) float64: the pair's gap -- squared: the sum over the axes
    of its square -- at a time drawn uniformly in the window clamped to the common domain, by trajectory_ref.forward_f64; about one in
    seven moved out of reach (the gap plus 1000; a thousandth of the squared one); 0 where there is no window."""
    rng = np.random.default_rng(seed)
    S, E = sr._domain(a, b, delay)[:2]
    with np.errstate(all="ignore"):
        t_lo, t_hi = np.maximum(lo, S), np.minimum(hi, E)
        ok = t_lo <= t_hi
        t = np.where(ok, t_lo + rng.uniform(size=ok.shape) * (t_hi - t_lo), 0.0)
        gaps = [tr.forward_f64(x, t)[0] - tr.forward_f64(y, t - delay)[0] for x, y in zip(a, b)]
        level = sum(g * g for g in gaps) if squared else gaps[0]
        away = rng.uniform(size=ok.shape) < 0.15
        level = np.where(away, level * 1e-3 if squared else level + 1e3, level)
        return np.ascontiguousarray(np.where(ok & np.isfinite(level), level, 0.0))


def _pair_queries(a, b, k, seed):
    """section 18's delays and windows of the random family: (lo, hi, delay)"""
    return gg._queries("random", a, b, lambda kk, s: gr.delays(a, b, kk, s), k, seed)


# ---------------------------------------------------------------- the families' comparisons with their definitions, on given rows
def _gap_against_the_definition(a, b, lo, hi, delay, got, what):
    """gap_gpu_cases.test_forward_against_the_definition's comparison for the random family.  got: gap_min, gap_max and their times."""
    k = lo.shape[1]
    sc, T = gr.scale(a, b), np.maximum(a[6] + a[7], b[6] + b[7])[:, None]
    want_v, want_t = gr.gap_ld(a, b, lo, hi, delay)
    lead = gr.runner_up_gap(a, b, lo, hi, delay)
    for j, name in enumerate(gr.NAMES):
        missing = np.isnan(want_v[j])
        clear = ~missing & (lead[j] >= 1e-9)
        left = float((~missing & ~clear).sum() / max((~missing).sum(), 1))
        if k > 1:
            assert left <= 0.01, (what, name, left)
        if got is None:      # the reference alone: the cap on what is left out
            print("%s %s: %.2f %% left out of the time comparison" % (what, name, 100 * left))
            continue
        got_v, got_t = got[j], got[2 + j]
        assert np.array_equal(np.isnan(got_v), missing) and np.array_equal(np.isnan(got_t), missing), (what, name, "the NaN mask")
        err = float(np.where(missing, 0, np.abs(got_v - want_v[j]) / sc).max())
        terr = float(np.where(clear, np.abs(got_t - want_t[j]) / T, 0).max())
        print("%s %s: value %.2e of the scale, time off ties %.2e, %.2f %% left out" % (what, name, err, terr, 100 * left))
        assert err <= 2e-13 and terr <= 1e-12, (what, name, err, terr)


def _tracking_against_the_definition(a, b, lo, hi, delay, got, what):
    """tracking_gpu_cases.test_forward_against_the_definition's comparison: tracking_ref.FORWARD_BOUNDS of the output's scale."""
    want = kr.tracking_ld(a, b, lo, hi, delay)
    walk = kr._walk(a, b, lo, hi, delay, LD)
    sc = kr.value_scales(a, b)
    for j, name in enumerate(kr.NAMES):
        missing = np.isnan(np.asarray(want[j], dtype=np.float64))
        assert np.array_equal(np.isnan(got[j]), missing), (what, name, "the NaN mask")
        assert np.all(got[j][walk["empty"]] == 0.0) and not np.any(np.signbit(got[j][walk["empty"]])), (what, name, "a == b")
        err = float(np.where(missing, 0, np.asarray(np.abs(got[j] - want[j]) / sc[j], dtype=np.float64)).max())
        print("%s %s: %.3g of the scale (bound %.3g)" % (what, name, err, kr.FORWARD_BOUNDS[j]))
        assert err <= kr.FORWARD_BOUNDS[j], (what, name, err)


def _meeting_against_the_definition(a, b, level, lo, hi, delay, got, what):
    """meeting_gpu_cases.test_forward_against_the_definition's comparison.  got: time, relvel."""
    time, relvel = got
    want, _, (t_lo, t_hi) = mr.meeting_ld(a, b, level, lo, hi, delay)
    reached = ~np.isnan(np.asarray(want, dtype=np.float64))
    assert np.array_equal(np.isnan(time), ~reached) and np.array_equal(np.isnan(relvel), ~reached), (what, "the NaN mask")
    T = mr.tmax(a, b, delay)
    assert np.all(((time >= t_lo - 4 * mr.EPS * T) & (time <= t_hi + 4 * mr.EPS * T))[reached]), (what, "the sub-piece")
    ratio, v_ld = mg._bound_c(a, b, level, delay, time, None)
    verr = np.where(reached, np.abs(relvel - v_ld), 0) / np.maximum(tr.scales(a)[1], tr.scales(b)[1])
    print("%s: %.1f %% reached, residual %.3f of (c), relvel %.2e of its scale" % (what, 100 * reached.mean(), ratio.max(), verr.max()))
    assert reached.any() and not reached.all(), what      # both kinds of answer on these rows
    assert float(ratio.max()) <= 1.0 and float(verr.max()) <= 2e-13, what


def _separation_against_the_definition(a, b, lo, hi, delay, got, what):
    """separation_gpu_cases.test_forward_against_the_definition's comparison for the random family and its cap on the share of boundary
    times left out (0.15 in one axis, 0.01 in more).  got: value, time -- or None: the reference alone, the cap."""
    d, k = len(a), lo.shape[1]
    cand = sr.candidates_ld(a, b, lo, hi, delay)
    want_v, want_t = sr.separation_ld(a, b, candidates=cand)
    lead = sr.runner_up(a, b, candidates=cand)
    missing = np.isnan(np.asarray(want_v, dtype=np.float64))
    cls = sr.classes(a, b, lo, hi, delay, np.asarray(want_t, dtype=np.float64))[0]
    boundary = ~missing & (cls != sr.OTHER)
    clear = boundary & (lead >= 1e-9)
    left = float((boundary & ~clear).sum() / max(boundary.sum(), 1))
    if k > 1:
        assert left <= (0.15 if d == 1 else sg.LEFT_OUT["random"]), (what, left)
    if got is None:
        print("%s: %.2f %% of the boundary times left out" % (what, 100 * left))
        return
    got_v, got_t = got
    assert np.array_equal(np.isnan(got_v), missing) and np.array_equal(np.isnan(got_t), missing), (what, "the NaN mask")
    f_at, gaps = sr.f_ld(a, b, np.where(missing, 0.0, got_t), np.where(missing, 0.0, delay))
    B = sr.value_bound(a, b, gaps)
    err = float(np.where(missing, 0, np.abs(got_v - f_at) / B).max())
    over = float(np.where(missing, 0, (f_at - want_v) / (2 * B)).max())
    assert _same_bits(got_t[clear], np.asarray(want_t, dtype=np.float64)[clear]), (what, "the bits of a boundary time")
    print("%s: value %.2e of B, over the minimum %.2e of 2 B, %.2f %% left out" % (what, err, over, 100 * left))
    assert err <= 1.0 and over <= 1.0, (what, err, over)


def _contact_against_the_definition(a, b, level, lo, hi, delay, got, what):
    """contact_gpu_cases.test_forward_against_the_definition's comparison.  got: time, rate."""
    time, rate = got
    want, _, (t_lo, t_hi) = cf.contact_ld(a, b, level, lo, hi, delay)
    missing = np.isnan(np.asarray(want, dtype=np.float64))
    assert np.array_equal(np.isnan(time), missing) and np.array_equal(np.isnan(rate), missing), (what, "the NaN mask")
    slack = 4 * cf.EPS * cf.tmax(a, b, delay)
    outside = ~missing & ((time < np.asarray(t_lo, dtype=np.float64) - slack) | (time > np.asarray(t_hi, dtype=np.float64) + slack))
    assert not outside.any(), (what, int(outside.sum()))
    f_at, bound = cg._bound_c(a, b, time, delay, missing)
    share = float(np.where(missing, 0, np.abs(f_at - level) / bound).max())
    print("%s: %.1f %% reached, residual %.3f of bound (c)" % (what, 100 * (~missing).mean(), share))
    assert missing.any() and not missing.all(), what      # both kinds of answer on these rows
    assert share <= 1.0, (what, share)


def _at(outputs, rows):
    return [x[rows] for x in outputs]


# ---------------------------------------------------------------- the pair entries
def test_gap():
    a, b = gr.random_pair(GRID_N)
    for k in KS:
        lo, hi, delay = _pair_queries(a, b, k, 840 + k)
        run, first = _kept(lambda *x: (lambda r: r[0] + r[1])(gg._gap(*x)))
        tg.rows_equal_their_own_batch(("gap", k), run, a, b, lo, hi, delay)
        _covered(first[0], ("gap", k))
        _gap_against_the_definition(_rows(a, MID), _rows(b, MID), lo[MID], hi[MID], delay[MID], _at(first[0], MID), "gap, k = %d" % k)


def test_tracking_forward():
    a, b = gr.random_pair(GRID_N)
    for k in KS:
        lo, hi, delay = _pair_queries(a, b, k, 850 + k)
        run, first = _kept(lambda *x: tk._track(*x))
        tg.rows_equal_their_own_batch(("tracking", k), run, a, b, lo, hi, delay)
        _covered(first[0], ("tracking", k))
        _tracking_against_the_definition(_rows(a, MID), _rows(b, MID), lo[MID], hi[MID], delay[MID], _at(first[0], MID), "tracking, k = %d" % k)


def test_tracking_vjp():
    """The reverse launch shape: G lanes per problem.  Against vjp_ld normwise, held to ten times the float64 restatement's worst error on
    the same rows (tracking_gpu_cases.test_vjp_and_jvp_against_longdouble's rule)."""
    a, b = gr.random_pair(GRID_N)
    for k in KS:
        lo, hi, delay = _pair_queries(a, b, k, 860 + k)
        g = tg._gradients(GRID_N, k, 861 + k)
        run, first = _kept(lambda *x: (lambda r: r[0] + r[1] + r[2])(tk._tvjp(*x)))
        tg.rows_equal_their_own_batch(("tracking vjp", k), run, a, b, lo, hi, delay, g)
        _covered(first[0], ("tracking vjp", k))
        args = (_rows(a, MID), _rows(b, MID), lo[MID], hi[MID], delay[MID], _rows(g, MID))
        stack = lambda v: list(v[0]) + list(v[1]) + list(v[2:] if len(v) == 5 else v[2])      # noqa: E731
        want, f64 = stack(kr.vjp_ld(*args)), stack(kr.vjp_f64(*args))
        got = _at(first[0], MID)
        assert all(np.isfinite(x).all() for x in got), (k, "a gradient is not finite")
        ref_err, dev_err = np.nanmax(tr.normwise(f64, want)), np.nanmax(tr.normwise(got, want))
        print("tracking vjp, k = %d: device %.3g, the float64 restatement %.3g" % (k, dev_err, ref_err))
        assert dev_err <= 10 * ref_err, (k, dev_err, ref_err)


def test_tracking_jvp():
    a, b = gr.random_pair(GRID_N)
    for k in KS:
        lo, hi, delay = _pair_queries(a, b, k, 870 + k)
        ad, bd, lod, hid, dld = tk._directions(GRID_N, k, 871 + k)
        run, first = _kept(lambda *x: tk._tjvp(*x))
        tg.rows_equal_their_own_batch(("tracking jvp", k), run, a, b, lo, hi, delay, ad, bd, lod, hid, dld)
        _covered(first[0], ("tracking jvp", k))
        args = (_rows(a, MID), _rows(b, MID), lo[MID], hi[MID], delay[MID], _rows(ad, MID), _rows(bd, MID), lod[MID], hid[MID], dld[MID])
        want, f64 = kr.jvp_ld(*args), kr.jvp_f64(*args)
        got = _at(first[0], MID)
        missing = np.isnan(np.asarray(want[0], dtype=np.float64))
        assert all(np.array_equal(np.isnan(x), missing) for x in got), (k, "the NaN mask of the tangents")
        z = lambda v: [np.where(missing, 0, x) for x in v]      # noqa: E731
        ref_err, dev_err = np.nanmax(tr.normwise(z(f64), z(want))), np.nanmax(tr.normwise(z(got), z(want)))
        print("tracking jvp, k = %d: device %.3g, the float64 restatement %.3g" % (k, dev_err, ref_err))
        assert dev_err <= 10 * ref_err, (k, dev_err, ref_err)


def _pair_levels(generate, plain, rows_list):
    """The stand-in levels with the family's own on the rows that meet the definition; generate(rows, j) -> (rows, k)"""
    level = plain
    for j, rows in enumerate(rows_list):
        level[rows] = generate(rows, j)
    return level


def meeting_inputs(k):
    a, b = gr.random_pair(GRID_N)
    lo, hi, delay = _pair_queries(a, b, k, 880 + k)
    level = _pair_levels(lambda rows, j: mr.levels(_rows(a, rows), _rows(b, rows), lo[rows], hi[rows], delay[rows], 882 + k + 10 * j)[0],
                         _plain_levels([a], [b], lo, hi, delay, 881 + k, squared=False), (MID,))
    return a, b, level, lo, hi, delay


def test_meeting():
    for k in KS:
        a, b, level, lo, hi, delay = meeting_inputs(k)
        run, first = _kept(lambda *x: list(mg._meeting(*x)))
        tg.rows_equal_their_own_batch(("meeting", k), run, a, b, level, lo, hi, delay)
        _covered(first[0], ("meeting", k))
        _meeting_against_the_definition(_rows(a, MID), _rows(b, MID), level[MID], lo[MID], hi[MID], delay[MID], _at(first[0], MID), "meeting, k = %d" % k)


def separation_inputs(k, d=2):
    a, b = sr.vehicles("random", GRID_N, d)
    delay = sr.delays(a, b, k, 890 + k)
    lo, hi = sr.windows(a, b, delay, 891 + k)
    return a, b, lo, hi, delay


def test_separation():
    for k in KS:
        a, b, lo, hi, delay = separation_inputs(k)
        run, first = _kept(lambda *x: sg._sep(*x))
        tg.rows_equal_their_own_batch(("separation", k), run, a, b, lo, hi, delay)
        _covered(first[0], ("separation", k))
        _separation_against_the_definition(_rows(a, MID), _rows(b, MID), lo[MID], hi[MID], delay[MID], _at(first[0], MID), "separation, k = %d" % k)


def contact_inputs(k, d=2):
    a, b, lo, hi, delay = separation_inputs(k, d)
    level = _pair_levels(lambda rows, j: cf.levels(_rows(a, rows), _rows(b, rows), lo[rows], hi[rows], delay[rows], 895 + k + 10 * j)[0],
                         _plain_levels(a, b, lo, hi, delay, 894 + k, squared=True), (MID,))
    return a, b, level, lo, hi, delay


def test_contact():
    for k in KS:
        a, b, level, lo, hi, delay = contact_inputs(k)
        run, first = _kept(lambda *x: cg._con(*x))
        tg.rows_equal_their_own_batch(("contact", k), run, a, b, level, lo, hi, delay)
        _covered(first[0], ("contact", k))
        _contact_against_the_definition(_rows(a, MID), _rows(b, MID), level[MID], lo[MID], hi[MID], delay[MID], _at(first[0], MID), "contact, k = %d" % k)


# ---------------------------------------------------------------- the fleet entries
def _mid_pairs(fleet, lo, hi):
    """the pair entry's view of the scenes around the second trip's start, the delay zeros"""
    a, b, rl, rh = fg.gathered(fg._scenes(fleet, MID_SCENES), lo[MID_SCENES], hi[MID_SCENES])
    return a, b, rl, rh, np.zeros(rl.shape)


def _flat(x):
    """(scenes, pairs, k) as the pair entry's (problems, k)"""
    return x.reshape(-1, x.shape[-1])


def test_fleet_separation(d):
    d = int(d)
    fleet = fg.fleet_inputs(SCENES, M, d)
    for k in KS:
        lo, hi = fg.scene_windows(fleet, k, 900 + k)
        full = scenes_equal_their_own_batch(("fleet separation", d, k), lambda *x: fg._fleet(*x), fleet, lo, hi)
        _covered(full, ("fleet separation", d, k))
        assert sg._all_same(full, fg._reference(fleet, lo, hi)), (d, k, "the pair entry on the gathered pairs")
        _separation_against_the_definition(*_mid_pairs(fleet, lo, hi), [_flat(x[MID_SCENES]) for x in full], "fleet separation, d = %d, k = %d" % (d, k))


def fleet_levels(fleet, lo, hi, d, k):
    """(per pair, per scene): fleet_contact_gpu_cases.levels_of on the scenes that meet the definition, the stand-in on the others"""
    a, b, rl, rh = fg.gathered(fleet, lo, hi)
    plain = _plain_levels(a, b, rl, rh, np.zeros(rl.shape), 300 + d + k, squared=True).reshape(SCENES, PAIRS, k)
    per_pair = _pair_levels(lambda rows, j: fc.levels_of(fg._scenes(fleet, rows), lo[rows], hi[rows], 300 + d + 10 * j)[0], plain, (MID_SCENES,))
    return per_pair, fc.scene_levels(per_pair)


def test_fleet_contact(layout, d):
    d = int(d)
    fleet = fg.fleet_inputs(SCENES, M, d)
    for k in KS:
        lo, hi = fg.scene_windows(fleet, k, 900 + k)
        level = fleet_levels(fleet, lo, hi, d, k)[fc.LAYOUTS.index(layout)]
        what = ("fleet contact", layout, d, k)
        full = scenes_equal_their_own_batch(what, lambda *x: fc._enc(*x), fleet, level, lo, hi)
        _covered(full, what)
        assert fc._all_same(full, fc._reference(fleet, level, lo, hi)), (what, "the pair entry on the gathered pairs")
        wide = level[MID_SCENES].reshape(-1, k) if level.ndim == 3 else np.repeat(level[MID_SCENES], PAIRS, axis=0)
        a, b, rl, rh, zero = _mid_pairs(fleet, lo, hi)
        _contact_against_the_definition(a, b, np.ascontiguousarray(wide), rl, rh, zero, [_flat(x[MID_SCENES]) for x in full],
                                        "fleet contact, level %s, d = %d, k = %d" % (layout, d, k))


def _mid_staggered(fleet, start, lo, hi):
    return si.gathered(fg._scenes(fleet, MID_SCENES), start[MID_SCENES], lo[MID_SCENES], hi[MID_SCENES])[:5]


def test_staggered_separation():
    d = 2
    fleet = fg.fleet_inputs(SCENES, M, d)
    start = si.starts_of(fleet)
    first, _ = fg.pairs_of(M)
    s_i = start[:, first][:, :, None]
    for k in KS:
        lo, hi = si.scene_windows(fleet, start, k, 900 + k)
        full = scenes_equal_their_own_batch(("staggered separation", k), lambda *x: st._stag(*x), fleet, start, lo, hi)
        _covered(full, ("staggered separation", k))
        want = st._ref_sep(fleet, start, lo, hi)
        assert _same_bits(full[0], want[0]) and _same_bits(full[2], want[2]), (k, "the pair entry on the gathered pairs")
        assert _same_bits(full[1], st._with_scene_time(full[2], s_i)) and _same_bits(full[1], want[1]), (k, "the scene's time")
        _separation_against_the_definition(*_mid_staggered(fleet, start, lo, hi), [_flat(full[f][MID_SCENES]) for f in (0, 2)],
                                           "staggered separation, k = %d" % k)


def staggered_levels(fleet, start, lo, hi, d, k):
    a, b, lo_p, hi_p, delay, _ = si.gathered(fleet, start, lo, hi)
    plain = _plain_levels(a, b, lo_p, hi_p, delay, 310 + d + k, squared=True).reshape(SCENES, PAIRS, k)
    per_pair = _pair_levels(lambda rows, j: st.levels_of(fg._scenes(fleet, rows), start[rows], lo[rows], hi[rows], 300 + d + 10 * j)[0], plain, (MID_SCENES,))
    return per_pair, fc.scene_levels(per_pair)


def test_staggered_contact():
    d = 2
    fleet = fg.fleet_inputs(SCENES, M, d)
    start = si.starts_of(fleet)
    first, _ = fg.pairs_of(M)
    s_i = start[:, first][:, :, None]
    for k in KS:
        lo, hi = si.scene_windows(fleet, start, k, 900 + k)
        for layout, level in zip(fc.LAYOUTS, staggered_levels(fleet, start, lo, hi, d, k)):
            what = ("staggered contact", layout, k)
            full = scenes_equal_their_own_batch(what, lambda *x: st._rdv(*x), fleet, start, level, lo, hi)
            _covered(full, what)
            want = st._ref_con(fleet, start, level, lo, hi)
            assert _same_bits(full[1], want[1]) and _same_bits(full[2], want[2]), (what, "the pair entry on the gathered pairs")
            assert _same_bits(full[0], st._with_scene_time(full[1], s_i)) and _same_bits(full[0], want[0]), (what, "the scene's time")
            a, b, lo_p, hi_p, delay = _mid_staggered(fleet, start, lo, hi)
            _contact_against_the_definition(a, b, np.ascontiguousarray(st._wide_level(level[MID_SCENES], PAIRS)), lo_p, hi_p, delay,
                                            [_flat(full[f][MID_SCENES]) for f in (1, 2)], "staggered contact, level %s, k = %d" % (layout, k))


def test_fleet_reach():
    """k_reach's boxes on 300,003 vehicles: rp_trajectory_extrema's pos_min and pos_max on the n m splines of each axis, bit for bit, as
    fleet_cull_gpu_cases.test_the_sieves_answer states it (the extrema kernel has section 13's case of its own beyond the cap)."""
    d = 2
    fleet = fg.fleet_inputs(SCENES, M, d)
    for k in KS:
        lo, hi = fg.scene_windows(fleet, k, 900 + k)
        full = scenes_equal_their_own_batch(("fleet reach", k), lambda f, l, h: (lambda r: r[0] + r[1])(fu._reach(f, l, h, k)), fleet, lo, hi)
        _covered(full, ("fleet reach", k))
        want = fu._extrema(fleet, lo, hi, k)
        assert sg._all_same(full, want[0] + want[1]), (k, "rp_trajectory_extrema on the same splines")
        print("fleet reach, k = %d: %d boxes the bits of rp_trajectory_extrema" % (k, full[0].size * d))


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
