"""The cases of tests/test_gpu_staggered.py, each run in a fresh process (`python tests/staggered_gpu_cases.py <case> [arguments]`), on top
of tests/fleet_gpu_cases.py's and tests/fleet_contact_gpu_cases.py's inputs.  Not collected by pytest (no test_ prefix on the file).  What is
checked, and why each bound is what it is: DESIGN.md section 28.  The reference throughout is the pair entry -- rp_trajectory_separation,
rp_trajectory_contact and their torch functions -- on the pairs gathered in numpy or torch with, for pair (i, j), the delay start_j -
start_i and the window [lo - start_i, hi - start_i], one float64 subtraction each."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_contact_gpu_cases as fc  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import contact_gpu_cases as cg  # noqa: E402
import contact_ref as cf  # noqa: E402
import fleet_gpu_cases as fg  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import separation_ref as sr  # noqa: E402
from staggered_inputs import gathered, input_shares, scene_windows, share_inside, starts_of  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

LD = np.longdouble
SIX, SHAPES = fg.SIX, fg.SHAPES
sg = fg.sg
_t, _bits, _same_bits, Out, _all_same = fg._t, fg._bits, fg._same_bits, fg.Out, fg.sg._all_same
fleet_inputs, pairs_of, _scenes = fg.fleet_inputs, fg.pairs_of, fg._scenes
CLASS_NAMES = ("LO", "HI", "END of the first", "END of the second", "START", "interior", "none")


def _stag(fleet, start, lo, hi, k=None, want=(True, True, True), zero_vel=False):
    """The staggered separation entry: [value, time, time_local], (n, pairs, k), None where not asked for."""
    n, m = start.shape
    d = len(fleet)
    k = k if k is not None else next(x for x in (lo, hi) if x is not None).shape[1]
    tf = [[_t(x) for x in axis] for axis in fleet]
    ts, tl, th = (_t(x) if x is not None else None for x in (start, lo, hi))
    outs = [Out(n, m * (m - 1) // 2, k) if w else None for w in want]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    capi.trajectory_fleet_separation_staggered(0, 0, n, m, k, d, addr, ts.data_ptr(), *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                               *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _rdv(fleet, start, level, lo, hi, want=(True, True, True), zero_vel=False):
    """The staggered contact entry: [time, time_local, rate], (n, pairs, k), None where not asked for.  A level of three dimensions goes in
    per pair, one of two per scene."""
    n, m = start.shape
    d, k = len(fleet), level.shape[-1]
    tf = [[_t(x) for x in axis] for axis in fleet]
    ts, tv, tl, th = (_t(x) if x is not None else None for x in (start, level, lo, hi))
    outs = [Out(n, m * (m - 1) // 2, k) if w else None for w in want]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    capi.trajectory_fleet_contact_staggered(0, 0, n, m, k, d, addr, ts.data_ptr(), tv.data_ptr(), int(level.ndim == 3),
                                            *[t.data_ptr() if t is not None else 0 for t in (tl, th)], *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _with_scene_time(local, s_i):
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(local + s_i)


def _ref_sep(fleet, start, lo, hi, k=None, **kw):
    """[value, time, time_local] of the pair entry on the gathered pairs, (n, pairs, k)"""
    n, m = start.shape
    a, b, lo_p, hi_p, delay, s_i = gathered(fleet, start, lo, hi, k)
    v, t = [x.reshape(n, m * (m - 1) // 2, -1) for x in sg._sep(a, b, lo_p, hi_p, delay, **kw)]
    return [v, _with_scene_time(t, s_i), t]


def _wide_level(level, pairs):
    return level.reshape(-1, level.shape[-1]) if level.ndim == 3 else np.repeat(level, pairs, axis=0)


def _ref_con(fleet, start, level, lo, hi, **kw):
    """[time, time_local, rate] of the pair entry on the gathered pairs, (n, pairs, k)"""
    n, m = start.shape
    pairs = m * (m - 1) // 2
    a, b, lo_p, hi_p, delay, s_i = gathered(fleet, start, lo, hi, level.shape[-1])
    t, r = [x.reshape(n, pairs, -1) for x in cg._con(a, b, np.ascontiguousarray(_wide_level(level, pairs)), lo_p, hi_p, delay, **kw)]
    return [_with_scene_time(t, s_i), t, r]


def levels_of(fleet, start, lo, hi, seed):
    """(the per-pair levels (n, pairs, k), the per-scene levels (n, k)): contact_ref.levels on the gathered pairs"""
    n, m = start.shape
    a, b, lo_p, hi_p, delay, _ = gathered(fleet, start, lo, hi)
    per_pair = cf.levels(a, b, lo_p, hi_p, delay, seed)[0].reshape(n, m * (m - 1) // 2, -1)
    return per_pair, fc.scene_levels(per_pair)


def _check_inputs(fleet, start, what):
    common, later = input_shares(fleet, start)
    print("%s: %.1f %% of the pairs have a common time, %.1f %% a delay > 0" % (what, 100 * common, 100 * later))
    assert 0.75 <= common <= 0.95 and 0.40 <= later <= 0.60, (what, common, later)


BAD_STARTS = ((3, (0,), np.nan), (9, (4,), np.inf), (17, (2,), -np.inf), (29, (1, 3), np.inf))      # scene, vehicles, value


def _poison(start, shape, k):
    """the four bad starts, and the pairs they must make NaN: exactly each vehicle's m - 1"""
    n, m = start.shape
    first, second = pairs_of(m)
    bad, poisoned = start.copy(), np.zeros(shape, dtype=bool)
    for s, vehicles, value in BAD_STARTS:
        for v in vehicles:
            bad[s, v] = value
            poisoned[s, (first == v) | (second == v), :] = True
    assert poisoned.sum() == (3 * (m - 1) + 2 * (m - 1) - 1) * k
    return bad, poisoned


def _bad_durations(fleet, shape, d):
    n, m = fleet[0][0].shape
    first, second = pairs_of(m)
    bad = [[x.copy() for x in axis] for axis in fleet]
    poisoned = np.zeros(shape, dtype=bool)
    for s, v, c, f, value in ((3, 0, 0, 6, 0.0), (9, 4, d - 1, 7, -1.0), (17, 2, 0, 7, np.inf), (29, 1, d - 1, 6, np.nan)):
        bad[c][f][s, v] = value
        poisoned[s, (first == v) | (second == v), :] = True
    return bad, poisoned


def _only_there(got, clean, poisoned, what):
    for x, ref in zip(got, clean):
        assert np.array_equal(np.isnan(x), poisoned | np.isnan(ref)), what
        assert np.array_equal(_bits(x[~poisoned]), _bits(ref[~poisoned])), what


# ---------------------------------------------------------------- 1. forward
def test_separation_is_the_pair_entry_bit_for_bit(shape):
    m, n, ks, ds = SHAPES[shape]
    inside = []
    for d in ds:
        fleet = fleet_inputs(n, m, d)
        start = starts_of(fleet)
        if shape != "64x1":      # (one scene is one draw of the shortest time: its shares are what they are; its launch is held to the 25 %)
            _check_inputs(fleet, start, "%s d = %d" % (shape, d))
        first, second = pairs_of(m)
        s_i = start[:, first][:, :, None]
        for k in ks:
            lo, hi = scene_windows(fleet, start, k, 900 + k)
            want = _ref_sep(fleet, start, lo, hi)
            got = _stag(fleet, start, lo, hi)
            assert _same_bits(got[0], want[0]) and _same_bits(got[2], want[2]), (shape, d, k)
            assert _same_bits(got[1], _with_scene_time(got[2], s_i)) and _same_bits(got[1], want[1]), (shape, d, k)
            share, finite = share_inside(fleet, start, lo, hi, want[0], want[2])
            inside.append(share)
            print("%s d = %d k = %d: %d queries the same bits in value, time and local time; %.0f %% finite, %.0f %% of those strictly inside "
                  "the window" % (shape, d, k, want[0].size, 100 * finite, 100 * share))
            if shape != "5x30" or k != 7:
                continue
            # a NULL window end is the infinite one, bit for bit; each output alone, nothing else written (the sentinels behind it)
            inf = np.full(lo.shape, np.inf)
            assert _all_same(_stag(fleet, start, None, hi), _stag(fleet, start, -inf, hi))
            assert _all_same(_stag(fleet, start, lo, None), _stag(fleet, start, lo, inf))
            assert _all_same(_stag(fleet, start, None, None, k=k), _stag(fleet, start, -inf, inf))
            assert _all_same(_stag(fleet, start, None, None, k=k), _ref_sep(fleet, start, None, None, k=k))
            for f in range(3):
                some = _stag(fleet, start, lo, hi, want=[g == f for g in range(3)])
                assert all(some[g] is None for g in range(3) if g != f) and _same_bits(some[f], got[f]), (d, f)
            # NULL end velocities are zeros
            still = [[x.copy() for x in axis] for axis in fleet]
            for axis in still:
                axis[3][:], axis[4][:] = 0.0, 0.0
            assert _all_same(_stag(still, start, lo, hi, zero_vel=True), _stag(still, start, lo, hi))
            assert _all_same(_stag(still, start, lo, hi, zero_vel=True), _ref_sep(still, start, lo, hi))
            # the NaN rule: a start of NaN, +inf, -inf, and both vehicles of a pair at +inf make exactly those vehicles' pairs NaN and change no
            # other bit; so do section 26's bad durations
            bad, poisoned = _poison(start, got[0].shape, k)
            _only_there(_stag(fleet, bad, lo, hi), got, poisoned, (d, "starts"))
            worse, poisoned = _bad_durations(fleet, got[0].shape, d)
            _only_there(_stag(worse, start, lo, hi), got, poisoned, (d, "durations"))
    print("%s: strictly inside the window: %s" % (shape, ", ".join("%.2f" % x for x in inside)))
    assert min(inside) >= 0.25, inside


def test_contact_is_the_pair_entry_bit_for_bit(shape, d):
    m, n, ks, _ = SHAPES[shape]
    d = int(d)
    fleet = fleet_inputs(n, m, d)
    start = starts_of(fleet)
    first, second = pairs_of(m)
    s_i = start[:, first][:, :, None]
    for k in ks:
        lo, hi = scene_windows(fleet, start, k, 900 + k)
        for layout, level in zip(fc.LAYOUTS, levels_of(fleet, start, lo, hi, 300 + d)):
            want = _ref_con(fleet, start, level, lo, hi)
            got = _rdv(fleet, start, level, lo, hi)
            finite = float(np.isfinite(want[1]).mean())
            assert np.array_equal(np.isnan(want[1]), np.isnan(want[2]))
            assert 0.0 < finite < 1.0, (shape, d, k, finite)      # both kinds of answer in every launch
            assert _same_bits(got[1], want[1]) and _same_bits(got[2], want[2]), (shape, d, k, layout)
            assert _same_bits(got[0], _with_scene_time(got[1], s_i)) and _same_bits(got[0], want[0]), (shape, d, k, layout)
            print("%s d = %d k = %d, level %s: %d queries the same bits in time, local time and rate; %.1f %% finite"
                  % (shape, d, k, layout, want[0].size, 100 * finite))
            if shape != "5x30" or k != 7:
                continue
            inf = np.full(lo.shape, np.inf)
            assert _all_same(_rdv(fleet, start, level, None, hi), _rdv(fleet, start, level, -inf, hi))
            assert _all_same(_rdv(fleet, start, level, lo, None), _rdv(fleet, start, level, lo, inf))
            assert _all_same(_rdv(fleet, start, level, None, None), _rdv(fleet, start, level, -inf, inf))
            assert _all_same(_rdv(fleet, start, level, None, None), _ref_con(fleet, start, level, None, None))
            for f in range(3):
                some = _rdv(fleet, start, level, lo, hi, want=[g == f for g in range(3)])
                assert all(some[g] is None for g in range(3) if g != f) and _same_bits(some[f], got[f]), (d, layout, f)
            still = [[x.copy() for x in axis] for axis in fleet]
            for axis in still:
                axis[3][:], axis[4][:] = 0.0, 0.0
            assert _all_same(_rdv(still, start, level, lo, hi, zero_vel=True), _rdv(still, start, level, lo, hi))
            assert _all_same(_rdv(still, start, level, lo, hi, zero_vel=True), _ref_con(still, start, level, lo, hi))
            bad, poisoned = _poison(start, got[0].shape, k)
            _only_there(_rdv(fleet, bad, level, lo, hi), got, poisoned, (d, layout, "starts"))
            worse, poisoned = _bad_durations(fleet, got[0].shape, d)
            _only_there(_rdv(worse, start, level, lo, hi), got, poisoned, (d, layout, "durations"))


# ---------------------------------------------------------------- 2. structure
def _translation_scene():
    """One scene of three vehicles in dyadic numbers (fleet_gpu_cases' first hand-made scene) with the starts 0, 0.5, 0.25: every sum with
    c = 4 is exact.  Pair (0, 1): the distance shrinks until the second vehicle ends, at 0.5 + 3 on the first's clock; pair (0, 2): it grows
    from the delayed start 0.25."""
    hand = [[np.ascontiguousarray(x[:1]) for x in axis] for axis in fg._hand_made_scene()]
    return hand, np.array([[0.0, 0.5, 0.25]])


def test_structure():
    m, n, k = 5, 30, 7
    for d in (1, 2, 3):
        fleet = fleet_inputs(n, m, d)
        start = starts_of(fleet)
        lo, hi = scene_windows(fleet, start, k, 950 + d)
        level = levels_of(fleet, start, lo, hi, 300 + d)[1]
        zeros = np.zeros((n, m))
        # a start of zeros: the bits of the entries without one
        z = _stag(fleet, zeros, lo, hi)
        assert _all_same([z[0], z[1]], fg._fleet(fleet, lo, hi)) and _same_bits(z[1], z[2]), d
        zc = _rdv(fleet, zeros, level, lo, hi)
        assert _all_same([zc[0], zc[2]], fc._enc(fleet, level, lo, hi)) and _same_bits(zc[0], zc[1]), d
        for run, args in ((lambda f, s, l, h, rows: _stag(f, s, l, h), "separation"), (lambda f, s, l, h, rows: _rdv(f, s, level[rows], l, h), "contact")):
            everything = slice(None)
            first = run(fleet, start, lo, hi, everything)
            assert _all_same(first, run(fleet, start, lo, hi, everything)), "differs from run to run"
            order = np.random.default_rng(5).permutation(n)
            assert _all_same(run(_scenes(fleet, order), start[order], lo[order], hi[order], order), [x[order] for x in first]), (d, args)
            for rows in (slice(0, 1), slice(12, 13), slice(29, 30), slice(n - 13, n)):      # single scenes, and the last 13 as a batch of their own
                part = run(_scenes(fleet, rows), np.ascontiguousarray(start[rows]), lo[rows], hi[rows], rows)
                assert _all_same(part, [x[rows] for x in first]), (d, args, rows)
        # the vehicles of a scene reversed: pair (i, j) becomes (m - 1 - j, m - 1 - i) on the other vehicle's clock, so the bits may differ;
        # each orientation is held to section 24's forward bound against the longdouble definition, as the pair entry is
        back = [[np.ascontiguousarray(x[:, ::-1]) for x in axis] for axis in fleet]
        start_back = np.ascontiguousarray(start[:, ::-1])
        got = _stag(back, start_back, lo, hi)
        a, b, lo_p, hi_p, delay, _ = gathered(back, start_back, lo, hi)
        want_v, _ = sr.separation_ld(a, b, lo_p, hi_p, delay)
        got_v, got_t = got[0].reshape(-1, k), got[2].reshape(-1, k)
        missing = np.isnan(np.asarray(want_v, dtype=np.float64))
        assert np.array_equal(np.isnan(got_v), missing), d
        f_at, gaps = sr.f_ld(a, b, np.where(missing, 0.0, got_t), np.where(missing, 0.0, delay))
        B = sr.value_bound(a, b, gaps)
        err = float(np.where(missing, 0, np.abs(got_v - f_at) / B).max())
        over = float(np.where(missing, 0, (f_at - want_v) / (2 * B)).max())
        pf, ps = pairs_of(m)
        where = {(i, j): p for p, (i, j) in enumerate(zip(pf, ps))}
        mirror = [where[(m - 1 - j, m - 1 - i)] for i, j in zip(pf, ps)]
        forward = _stag(fleet, start, lo, hi)[0][:, mirror, :].reshape(-1, k)
        assert np.array_equal(np.isnan(forward), missing), d
        apart = float(np.where(missing, 0, np.abs(forward - got_v) / B).max())
        print("d = %d, vehicles reversed: value %.2e of B, over the minimum %.2e of 2 B; %.2e of B from the other orientation, %.1f %% other bits"
              % (d, err, over, apart, 100 * float((_bits(forward) != _bits(got_v)).mean())))
        assert err <= 1.0 and over <= 1.0
    # translation: adding 4 to every start, lo and hi of a dyadic scene moves the scene-clock times by exactly 4 and nothing else
    hand, start = _translation_scene()
    lo, hi = np.array([[-np.inf, 0.125, 0.5]]), np.array([[np.inf, 8.0, 3.25]])
    here, there = _stag(hand, start, lo, hi), _stag(hand, start + 4.0, lo + 4.0, hi + 4.0)
    print("hand-made scene: local times %s" % here[2].ravel())
    assert np.isfinite(here[0]).all()
    assert _same_bits(here[0], there[0]) and _same_bits(here[2], there[2]) and _same_bits(here[1] + 4.0, there[1])
    assert here[2][0, 0, 0] == 3.5 and here[2][0, 1, 0] == 0.25
    print("the same bits in any order of the scenes and in any batch; zeros are the entries without a start")


# ---------------------------------------------------------------- 3. autograd
def _expanded(splines, start, lo, hi, m):
    """The pair entry's leaves from eight (n, m, d) tensors, start (n, m), lo and hi (n, k): A (8), B (8), s_i, s_j (n pairs, 1), lo, hi
    (n pairs, k) -- detached, so that each pair's terms stay apart -- and the composed delay, lo', hi'."""
    n, _, d = splines[0].shape
    k = lo.shape[1]
    first, second = (torch.as_tensor(x, device=splines[0].device) for x in pairs_of(m))
    wide = lambda t, which: t.detach()[:, which, :].reshape(-1, d).clone().requires_grad_()      # noqa: E731
    a, b = [wide(t, first) for t in splines], [wide(t, second) for t in splines]
    s_i = start.detach()[:, first].reshape(-1, 1).clone().requires_grad_()
    s_j = start.detach()[:, second].reshape(-1, 1).clone().requires_grad_()
    rep = lambda w: w.detach().unsqueeze(1).expand(n, len(first), k).reshape(-1, k).clone().requires_grad_()      # noqa: E731
    lo_e, hi_e = rep(lo), rep(hi)
    delay = (s_j - s_i).expand(-1, k)
    return a, b, s_i, s_j, lo_e, hi_e, delay, lo_e - s_i, hi_e - s_i


def _fold_starts(term_i, term_j, n, m):
    first, second = pairs_of(m)
    out = np.zeros((n, m), dtype=LD)
    np.add.at(out, (slice(None), first), term_i.reshape(n, len(first)))
    np.add.at(out, (slice(None), second), term_j.reshape(n, len(first)))
    return out


def _reference_gradients(out, leaves, g, n, m, d, k, extra):
    """One backward per query column of the pair entry's `out` (n pairs, k), the terms added in longdouble.  leaves: A (8), B (8), s_i, s_j,
    then `extra` per-query leaves (n pairs, k) or (n, k)-foldable.  Returns (total, size) lists: the eight (n, m, d), start (n, m), then
    per extra leaf (n, pairs, k); and per column the start's and the extras' sizes, for the translation identity."""
    pairs = m * (m - 1) // 2
    total = [np.zeros((n, m, d), dtype=LD) for _ in range(8)] + [np.zeros((n, m), dtype=LD)] + [np.zeros((n, pairs, k), dtype=LD) for _ in range(extra)]
    size = [np.zeros_like(x) for x in total]
    start_size_by_column = []
    for q in range(k):
        column = torch.zeros_like(out)
        column[:, q] = g.reshape(-1, k)[:, q]
        terms = [x.cpu().numpy().astype(LD) if x is not None else None
                 for x in torch.autograd.grad(out, leaves, grad_outputs=column, retain_graph=True, allow_unused=True)]
        for f in range(8):
            total[f] += fg._folded(terms[f], terms[8 + f], n, m)
            size[f] += fg._folded(np.abs(terms[f]), np.abs(terms[8 + f]), n, m)
        total[8] += _fold_starts(terms[16], terms[17], n, m)
        by_column = _fold_starts(np.abs(terms[16]), np.abs(terms[17]), n, m)
        size[8] += by_column
        start_size_by_column.append(by_column)
        for x in range(extra):
            if terms[18 + x] is not None:
                total[9 + x] += terms[18 + x].reshape(n, pairs, k)
                size[9 + x] += np.abs(terms[18 + x]).reshape(n, pairs, k)
    return total, size, start_size_by_column


def _assert_close(got, total, size, what):
    """fleet_gpu_cases._assert_close with the start: the eight gradients of a vehicle and axis share the largest of their eight sums of
    |terms| as the unit (its reason); the start of a vehicle takes its tau_bar from every axis' launch of the same kernel, so its unit is
    the largest sum of |terms| of the vehicle: over its own, and its eight gradients of every axis.  The others: the element's own."""
    shared = np.max(np.stack(size[:8]), axis=0)
    vehicle = np.maximum(size[8], shared.max(axis=2))
    worst = 0.0
    for f, (x, ref, s) in enumerate(zip(got, total, size)):
        s = shared if f < 8 else vehicle if f == 8 else s
        err = np.abs(x.astype(LD) - ref)
        ratio = float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1), 0)))
        print("  %s, input %d: at most %.2e of the sum of |terms|" % (what, f, ratio))
        worst = max(worst, ratio)
        assert np.all(err <= 1e-12 * s), (what, f, float(np.max(err - 1e-12 * s)))
    return worst


def _duality(got, dots, g, got_dot, ref_dot, what):
    gn, dn = g.cpu().numpy(), [t.cpu().numpy() for t in dots]
    left_terms = [np.where(np.isnan(got_dot), 0, gn.astype(LD) * got_dot)]
    right_terms = [x.astype(LD) * t for x, t in zip(got, dn)]
    left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
    scale = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
    ref_left = float(np.where(np.isnan(ref_dot), 0, gn.astype(LD) * ref_dot).sum())
    print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|; forward mode against the pair entry's: %.2e"
          % (what, abs(left - right) / scale, abs(left - ref_left) / scale))
    assert abs(left - right) <= 1e-12 * scale and abs(left - ref_left) <= 1e-12 * scale
    assert np.array_equal(np.isnan(ref_dot), np.isnan(got_dot))


def _raises_on_double_backward(loss, leaf):
    (g0,) = torch.autograd.grad(loss(), leaf, create_graph=True)
    try:
        g0.sum().backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("double backward did not raise")


def test_separation_autograd_against_the_pair_entry(d):
    d = int(d)
    m, n, k = 5, 30, 7
    pairs = m * (m - 1) // 2
    fleet = fleet_inputs(n, m, d)
    start_np = starts_of(fleet)
    lo_np, hi_np = scene_windows(fleet, start_np, k, 960 + d)
    leaves = fg._fleet_leaves(fleet)
    start, lo, hi = (_t(x).requires_grad_() for x in (start_np, lo_np, hi_np))
    rng = np.random.default_rng(961)
    g = _t(rng.standard_normal((n, pairs, k)))
    run = lambda lv, s, l, h: rp.trajectory_fleet_separation([lv[f] for f in SIX], l, h, start=s)      # noqa: E731
    outs = run(leaves, start, lo, hi)
    assert len(outs) == 2 and outs[0].requires_grad and not outs[1].requires_grad
    every = leaves + [start, lo, hi]
    a, b, s_i, s_j, lo_e, hi_e, delay, lo_p, hi_p = _expanded(leaves, start, lo, hi, m)
    ref = rp.trajectory_separation([a[f] for f in SIX], [b[f] for f in SIX], lo_p, hi_p, delay)
    assert _same_bits(outs[0].detach().cpu().numpy().reshape(-1, k), ref[0].detach().cpu().numpy())
    assert _same_bits(outs[1].cpu().numpy().reshape(-1, k), (ref[1] + s_i.detach()).cpu().numpy())
    total, size, by_column = _reference_gradients(ref[0], a + b + [s_i, s_j, lo_e, hi_e], g, n, m, d, k, 2)
    # the classes of the returned times, on the pair entry's times: all seven
    an, bn, lo_n, hi_n, delay_n, _ = gathered(fleet, start_np, lo_np, hi_np)
    cls = sr.classes(an, bn, lo_n, hi_n, delay_n, ref[1].cpu().numpy())[0]
    share = np.bincount(cls.ravel(), minlength=7) / cls.size
    print("d = %d: classes of the returned times: %s" % (d, ", ".join("%s %.3f" % x for x in zip(CLASS_NAMES, share))))
    assert np.all(share > 0), share
    got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    again = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
    assert all(np.isfinite(x).all() for x in got)
    fold = lambda x: x.sum(axis=1)      # noqa: E731  lo and hi: a scene's window holds for all its pairs
    worst = _assert_close(got, total[:9] + [fold(total[9]), fold(total[10])], size[:9] + [fold(size[9]), fold(size[10])], "reverse mode")
    print("d = %d: reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, asserted 1e-12" % (d, worst))
    assert np.abs(got[8]).max() > 0
    # translation invariance: per scene and query the starts', lo's and hi's gradients sum to 0
    worst = 0.0
    for q in range(k):
        column = torch.zeros_like(g)
        column[:, :, q] = g[:, :, q]
        s_bar, l_bar, h_bar = (x.cpu().numpy().astype(LD) for x in torch.autograd.grad(outs[0], [start, lo, hi], grad_outputs=column, retain_graph=True))
        assert np.all(np.delete(l_bar, q, axis=1) == 0) and np.all(np.delete(h_bar, q, axis=1) == 0)
        unit = by_column[q].sum(axis=1) + fold(size[9])[:, q] + fold(size[10])[:, q]
        left = np.abs(s_bar.sum(axis=1) + l_bar[:, q] + h_bar[:, q])
        worst = max(worst, float(np.max(np.where(unit > 0, left / np.where(unit > 0, unit, 1), 0))))
        assert np.all(left <= 1e-12 * unit), (q, float(np.max(left - 1e-12 * unit)))
    print("d = %d: the gradients in the starts, lo and hi sum to 0 per scene and query: at most %.2e of the sum of |terms|, asserted 1e-12" % (d, worst))
    # a NaN value has gradient exactly 0
    miss = torch.isnan(outs[0].detach())
    assert int(miss.sum()) > 0
    for x in torch.autograd.grad(outs[0], every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
        assert float(x.abs().max()) == 0.0
    # forward mode, torch.func.jvp, duality, and the pair entry's forward mode on the gathered pairs
    dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal((n, m)))] + [_t(rng.standard_normal((n, k))) for _ in range(2)]
    with fwAD.dual_level():
        dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
        douts = run(dual[:8], dual[8], dual[9], dual[10])
        got_dot = fwAD.unpack_dual(douts[0]).tangent.cpu().numpy()
        assert fwAD.unpack_dual(douts[1]).tangent is None
    _, func_dot = torch.func.jvp(lambda *xs: run(list(xs[:8]), xs[8], xs[9], xs[10])[0], tuple(x.detach() for x in every), tuple(dots))
    assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
    first, second = (torch.as_tensor(x, device=g.device) for x in pairs_of(m))
    gather = lambda t, which: t[:, which, :].reshape(-1, d)      # noqa: E731
    with fwAD.dual_level():
        dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
        pa, pb = [gather(t, first) for t in dual[:8]], [gather(t, second) for t in dual[:8]]
        di, dj = dual[8][:, first].reshape(-1, 1), dual[8][:, second].reshape(-1, 1)
        rep = lambda w: w.unsqueeze(1).expand(n, pairs, k).reshape(-1, k)      # noqa: E731
        ref_dot = fwAD.unpack_dual(rp.trajectory_separation([pa[f] for f in SIX], [pb[f] for f in SIX], rep(dual[9]) - di, rep(dual[10]) - di,
                                                            (dj - di).expand(-1, k))[0]).tangent
        ref_dot = ref_dot.cpu().numpy().reshape(got_dot.shape)
    _duality(got, dots, g, got_dot, ref_dot, "d = %d" % d)
    _raises_on_double_backward(lambda: (torch.nan_to_num(run(leaves, start, lo, hi)[0]) ** 2).sum(), start)
    if d != 2:
        torch.cuda.synchronize()
        return
    # the hand-made dyadic scene: pair (0, 1) ends with its second vehicle, pair (0, 2) starts with the delayed one; both move with the starts
    hand, hs = _translation_scene()
    hl = fg._fleet_leaves(hand)
    h_start = _t(hs).requires_grad_()
    whole = np.full((1, 1), np.inf)
    outs = run(hl, h_start, None, None)
    an, bn, lo_n, hi_n, delay_n, s_n = gathered(hand, hs, -whole, whole)
    local = outs[1].cpu().numpy() - s_n
    cls = sr.classes(an, bn, lo_n, hi_n, delay_n, local.reshape(3, 1))[0]
    print("hand-made scene: local times %s, classes %s" % (local.ravel(), cls.ravel()))
    assert cls[0, 0] == sr.END_B and cls[1, 0] == sr.START and local[0, 0, 0] == 3.5 and local[0, 1, 0] == 0.25
    inf = _t(whole)
    a, b, s_i, s_j, lo_e, hi_e, delay, lo_p, hi_p = _expanded(hl, h_start, -inf, inf, 3)
    ref = rp.trajectory_separation([a[f] for f in SIX], [b[f] for f in SIX], lo_p, hi_p, delay)
    total, size, _ = _reference_gradients(ref[0], a + b + [s_i, s_j], torch.ones_like(outs[0]), 1, 3, 2, 1, 0)
    got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0].sum(), hl + [h_start])]
    _assert_close(got, total, size, "hand-made scene")
    for keep in ((0,), (1,)):      # each pair alone: its two vehicles' starts get a gradient that is not 0
        pick = torch.zeros_like(outs[0])
        pick[0, keep[0], 0] = 1.0
        (s_bar,) = torch.autograd.grad(run(hl, h_start, None, None)[0], h_start, grad_outputs=pick)
        print("hand-made scene, pair %d alone: start_bar %s" % (keep[0], s_bar.cpu().numpy().ravel()))
        assert s_bar[0, 0].item() != 0 and s_bar[0, 1 + keep[0]].item() != 0 and s_bar[0, 2 - keep[0]].item() == 0
        assert s_bar.sum().item() == 0      # no window: the value depends on the difference of the two starts only
    torch.cuda.synchronize()


def test_contact_autograd_against_the_pair_entry(d):
    d = int(d)
    m, n, k = 5, 30, 7
    pairs = m * (m - 1) // 2
    fleet = fleet_inputs(n, m, d)
    start_np = starts_of(fleet)
    lo_np, hi_np = scene_windows(fleet, start_np, k, 960 + d)
    rng = np.random.default_rng(961)
    g = _t(rng.standard_normal((n, pairs, k)))
    run = lambda lv, s, level, radius=None: rp.trajectory_fleet_contact([lv[f] for f in SIX], radius, lo, hi, level_sq=level, start=s)      # noqa: E731
    lo, hi = _t(lo_np), _t(hi_np)
    for layout, level_np in zip(fc.LAYOUTS, levels_of(fleet, start_np, lo_np, hi_np, 300 + d)):
        leaves = fg._fleet_leaves(fleet)
        start = _t(start_np).requires_grad_()
        radius_np = np.sqrt(np.abs(level_np)) + 0.125
        for by_radius, query_np in ((False, level_np), (True, radius_np)):
            query = _t(query_np).requires_grad_()
            out = run(leaves, start, None, query) if by_radius else run(leaves, start, query)
            assert isinstance(out, torch.Tensor) and out.shape == (n, pairs, k) and out.requires_grad
            every = leaves + [start, query]
            a, b, s_i, s_j, _, _, delay, lo_p, hi_p = _expanded(leaves, start, lo, hi, m)
            query_e = fc._wide_level(query.detach(), pairs).clone().requires_grad_()
            local = rp.trajectory_contact([a[f] for f in SIX], [b[f] for f in SIX], query_e if by_radius else None, lo_p.detach(), hi_p.detach(), delay,
                                          level_sq=None if by_radius else query_e)
            ref = torch.where(torch.isnan(local), local, local + s_i)      # an unreached level stays NaN and sends nothing to the start
            assert _same_bits(out.detach().cpu().numpy().reshape(-1, k), ref.detach().cpu().numpy())
            miss = torch.isnan(out.detach())
            share = float(miss.double().mean())
            assert 0.05 <= share <= 0.95, share
            total, size, by_column = _reference_gradients(ref, a + b + [s_i, s_j, query_e], g, n, m, d, k, 1)
            grads = torch.autograd.grad(out, every, grad_outputs=g, retain_graph=True)
            got = [x.cpu().numpy() for x in grads]
            again = [x.cpu().numpy() for x in torch.autograd.grad(out, every, grad_outputs=g, retain_graph=True)]
            assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
            assert all(np.isfinite(x).all() for x in got) and got[9].shape == query_np.shape
            fold = (lambda x: x) if query_np.ndim == 3 else (lambda x: x.sum(axis=1))      # noqa: E731
            what = "%s %s" % ("radius" if by_radius else "level", layout)
            worst = _assert_close(got, total[:9] + [fold(total[9])], size[:9] + [fold(size[9])], "reverse mode, " + what)
            print("d = %d, %s: reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, asserted "
                  "1e-12; %.1f %% unreached" % (d, what, worst, 100 * share))
            # translation: the starts' gradients of a scene sum to the upstream gradients of its reached queries (the time moves with the clock)
            want = np.where(miss.cpu().numpy(), 0, g.cpu().numpy().astype(LD)).sum(axis=(1, 2))
            unit = size[8].sum(axis=1) + np.where(miss.cpu().numpy(), 0, np.abs(g.cpu().numpy())).sum(axis=(1, 2))
            assert np.all(np.abs(got[8].astype(LD).sum(axis=1) - want) <= 1e-12 * unit)
            for x in torch.autograd.grad(out, every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
                assert float(x.abs().max()) == 0.0      # an unreached level has gradient exactly 0
            if by_radius:
                continue
            dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal((n, m))), _t(rng.standard_normal(level_np.shape))]
            with fwAD.dual_level():
                dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
                got_dot = fwAD.unpack_dual(run(dual[:8], dual[8], dual[9])).tangent.cpu().numpy()
            _, func_dot = torch.func.jvp(lambda *xs: run(list(xs[:8]), xs[8], xs[9]), tuple(x.detach() for x in every), tuple(dots))
            assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
            first, second = (torch.as_tensor(x, device=g.device) for x in pairs_of(m))
            gather = lambda t, which: t[:, which, :].reshape(-1, d)      # noqa: E731
            with fwAD.dual_level():
                dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
                pa, pb = [gather(t, first) for t in dual[:8]], [gather(t, second) for t in dual[:8]]
                di, dj = dual[8][:, first].reshape(-1, 1), dual[8][:, second].reshape(-1, 1)
                rep = lambda w: w.unsqueeze(1).expand(n, pairs, k).reshape(-1, k)      # noqa: E731
                ref_t = rp.trajectory_contact([pa[f] for f in SIX], [pb[f] for f in SIX], None, rep(lo) - di, rep(hi) - di, (dj - di).expand(-1, k),
                                              level_sq=fc._wide_level(dual[9], pairs))
                ref_t = torch.where(torch.isnan(ref_t), ref_t, ref_t + di)
                ref_dot = fwAD.unpack_dual(ref_t).tangent.cpu().numpy().reshape(got_dot.shape)
            _duality(got, dots, g, got_dot, ref_dot, "d = %d, level %s" % (d, layout))
            _raises_on_double_backward(lambda: (torch.nan_to_num(run(leaves, start, query)) ** 2).sum(), start)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. through the solves
def test_the_pipeline_is_the_composition():
    """min_time_fleet_separation and min_time_fleet_contact with start= (m = 3, d = 2, n = 100, k = 8, synchronised) on golden problems: the
    bits of min_time_solve + synchronize_axes + the fleet function composed by hand; the gradients in pos1 and start finite, and within
    1e-12 of the sum of |terms| of the same composition with the pair entry on the gathered pairs (fleet_gpu_cases' units: a term is one
    (pair, query)'s share, the unit of pos1 the largest sum among the vehicle's axes, the unit of a start the vehicle's largest)."""
    n, m, d, k = 100, 3, 2, 8
    pairs = m * (m - 1) // 2
    pos = gg._golden_positions(n * m * d).reshape(n, m, d, 3)
    x = [_t(pos[..., c]).requires_grad_() for c in range(3)]

    def spline_of(p):
        sol = rp.min_time_solve(*[t.reshape(-1) for t in p], gap_tol=1e-13)
        six, _ = rp.synchronize_axes([t.reshape(n * m, d) for t in list(p) + [s.reshape(n, m, d) for s in sol[:3]]])
        return [t.reshape(n, m, d) for t in six], sol

    with torch.no_grad():
        six, sol = spline_of(x)
    z = np.zeros((n, m))
    st = [t.detach().cpu().numpy() for t in six]
    good = np.isfinite(np.stack(st, 3)).all(axis=(1, 2, 3))
    fleet_np = [[np.where(good[:, None], v, 1.0) for v in (st[0][..., c], st[1][..., c], st[2][..., c], z, z, st[3][..., c], st[4][..., c], st[5][..., c])]
                for c in range(d)]
    start_np = starts_of(fleet_np)
    lo_np, hi_np = scene_windows(fleet_np, start_np, k, 970)
    lo, hi = _t(lo_np), _t(hi_np)
    start = _t(start_np).requires_grad_()
    level = _t(levels_of(fleet_np, start_np, lo_np, hi_np, 302)[0])      # per pair: a scene's one level is reached by too few of its pairs
    first, second = pairs_of(m)
    table = (0, 1, 2, 5, 6, 7)      # the six of synchronize_axes in the table's order
    ok_rows = good[:, None, None] & np.ones((n, m, d), dtype=bool)
    for what in ("separation", "contact"):
        if what == "separation":
            out = rp.min_time_fleet_separation(x, lo, hi, gap_tol=1e-13, start=start)
            assert len(out) == 3 and len(out[2]) == 5
            value, solution = out[0], out[2]
        else:
            out = rp.min_time_fleet_contact(x, None, lo, hi, level_sq=level, gap_tol=1e-13, start=start)
            assert len(out) == 2 and len(out[1]) == 5
            value, solution = out
        six, sol = spline_of(x)
        if what == "separation":
            by_hand = rp.trajectory_fleet_separation(six, lo, hi, start=start)
            assert _same_bits(out[1].cpu().numpy(), by_hand[1].cpu().numpy())
            by_hand = by_hand[0]
        else:
            by_hand = rp.trajectory_fleet_contact(six, None, lo, hi, level_sq=level, start=start)
        assert _same_bits(value.detach().cpu().numpy(), by_hand.detach().cpu().numpy())
        assert all(_same_bits(p.detach().cpu().numpy().astype(np.float64), q.detach().cpu().numpy().reshape(n, m, d).astype(np.float64))
                   for p, q in zip(solution, sol))
        finite = torch.isfinite(value.detach())
        print("%s: %d of %d scenes solved finite, %.0f %% of the queries finite" % (what, int(good.sum()), n, 100 * float(finite.double().mean())))
        assert good.mean() > 0.95 and float(finite.double().mean()) >= 0.25
        g = _t(np.random.default_rng(971).uniform(0.5, 1.5, tuple(value.shape)))
        g = torch.where(finite, g, torch.zeros_like(g))
        got, got_start = torch.autograd.grad(value, [x[1], start], grad_outputs=g)
        ok = _t(good).bool()
        assert torch.isfinite(got[ok[:, None, None].expand_as(got)]).all() and torch.isfinite(got_start[ok[:, None].expand_as(got_start)]).all()
        eight = six[:3] + [torch.zeros_like(six[0]), torch.zeros_like(six[0])] + six[3:]
        a, b, s_i, s_j, _, _, delay, lo_p, hi_p = _expanded(eight, start, lo, hi, m)
        if what == "separation":
            ref = rp.trajectory_separation([a[f] for f in SIX], [b[f] for f in SIX], lo_p, hi_p, delay)[0]
        else:
            ref = rp.trajectory_contact([a[f] for f in SIX], [b[f] for f in SIX], None, lo_p.detach(), hi_p.detach(), delay,
                                        level_sq=fc._wide_level(level, pairs).contiguous())
            ref = torch.where(torch.isnan(ref), ref, ref + s_i)      # an unreached level stays NaN and sends nothing to the start
        assert _same_bits(ref.detach().cpu().numpy().reshape(n, pairs, k), by_hand.detach().cpu().numpy())
        total, size = np.zeros((n, m, d), dtype=LD), np.zeros((n, m, d), dtype=LD)
        total_s, size_s = np.zeros((n, m), dtype=LD), np.zeros((n, m), dtype=LD)
        g_flat = g.reshape(n * pairs, k)
        for q in range(k):
            column = torch.zeros_like(ref)
            column[:, q] = g_flat[:, q]
            terms = torch.autograd.grad(ref, [a[f] for f in table] + [b[f] for f in table] + [s_i, s_j], grad_outputs=column, retain_graph=True)
            t_i, t_j = (t.cpu().numpy().astype(LD) for t in terms[12:])
            total_s += _fold_starts(t_i, t_j, n, m)
            size_s += _fold_starts(np.abs(t_i), np.abs(t_j), n, m)
            for p in range(pairs):
                bars = []
                for f in range(6):
                    bar = torch.zeros((n, m, d), dtype=torch.float64, device=g.device)
                    bar[:, first[p], :] = terms[f].reshape(n, pairs, d)[:, p, :]
                    bar[:, second[p], :] = terms[6 + f].reshape(n, pairs, d)[:, p, :]
                    bars.append(bar)
                (term,) = torch.autograd.grad(six, x[1], grad_outputs=bars, retain_graph=True)
                term = term.cpu().numpy().astype(LD)
                total += term
                size += np.abs(term)
        size = np.repeat(size.max(axis=2, keepdims=True), d, axis=2)      # the stretch to the slowest axis couples a vehicle's axes: their largest
        err = np.abs(got.cpu().numpy().astype(LD) - total)
        worst = float(np.max(np.where(ok_rows & (size > 0), err / np.where(size > 0, size, 1), 0)))
        err_s = np.abs(got_start.cpu().numpy().astype(LD) - total_s)
        worst_s = float(np.max(np.where(good[:, None] & (size_s > 0), err_s / np.where(size_s > 0, size_s, 1), 0)))
        print("%s through the pipeline against the same composition with the pair entry: pos1 at most %.2e, start at most %.2e of the sum of "
              "|terms|, asserted 1e-12" % (what, worst, worst_s))
        assert np.all(err[ok_rows] <= 1e-12 * size[ok_rows]) and np.all(err_s[good] <= 1e-12 * size_s[good])
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
