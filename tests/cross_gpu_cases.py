"""The cases of tests/test_gpu_cross.py, each run in a fresh process (`python tests/cross_gpu_cases.py <case> [arguments]`), on top of
tests/cross_inputs.py's inputs and the pair entries of tests/separation_gpu_cases.py and tests/contact_gpu_cases.py.  Not collected by
pytest (no test_ prefix on the file).  What is checked, and why each bound is what it is: DESIGN.md section 34.  The reference throughout
is the pair entry -- rp_trajectory_separation / rp_trajectory_contact, trajectory_separation / trajectory_contact -- on the m_a m_b pairs
of every scene gathered in numpy or torch, with the scene's windows -- and a per-scene level -- repeated per pair and the delay NULL."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_gpu_cases as fg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import contact_gpu_cases as cg  # noqa: E402
import cross_inputs as ci  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import separation_gpu_cases as sg  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

LD = np.longdouble
SIX, SHAPES, LAYOUTS = fg.SIX, ci.SHAPES, ("per pair", "per scene")
_t, _bits, _same_bits, Out, _all_same = fg._t, fg._bits, fg._same_bits, fg.Out, sg._all_same


def _sizes(fleet_a, fleet_b):
    return fleet_a[0][0].shape[0], fleet_a[0][0].shape[1], fleet_b[0][0].shape[1], len(fleet_a)


def _tables(fleet_a, fleet_b, zero_vel):
    """(the tensors, kept alive by the caller; the two lists of 8 d addresses)"""
    keep = [[[_t(x) for x in axis] for axis in fleet] for fleet in (fleet_a, fleet_b)]
    return keep, [[0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in fleet for f, t in enumerate(axis)] for fleet in keep]


def _vs(fleet_a, fleet_b, lo, hi, k=None, want=(True, True), zero_vel=False):
    """rp_trajectory_cross_separation: (value, time), (n, pairs, k), None where not asked for.  lo / hi of None go in as NULL."""
    n, m_a, m_b, d = _sizes(fleet_a, fleet_b)
    k = k if k is not None else next(x for x in (lo, hi) if x is not None).shape[1]
    keep, addr = _tables(fleet_a, fleet_b, zero_vel)
    tl, th = (_t(x) if x is not None else None for x in (lo, hi))
    outs = [Out(n, m_a * m_b, k) if w else None for w in want]
    capi.trajectory_cross_separation(0, 0, n, m_a, m_b, k, d, addr[0], addr[1], *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                     *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _icp(fleet_a, fleet_b, level, lo, hi, want_rate=True, zero_vel=False):
    """rp_trajectory_cross_contact: (time, rate), (n, pairs, k), rate None where not asked for.  A level of three dimensions goes in per
    pair, one of two per scene; lo / hi of None go in as NULL."""
    n, m_a, m_b, d = _sizes(fleet_a, fleet_b)
    k = level.shape[-1]
    keep, addr = _tables(fleet_a, fleet_b, zero_vel)
    tv, tl, th = (_t(x) if x is not None else None for x in (level, lo, hi))
    outs = [Out(n, m_a * m_b, k), Out(n, m_a * m_b, k) if want_rate else None]
    capi.trajectory_cross_contact(0, 0, n, m_a, m_b, k, d, addr[0], addr[1], tv.data_ptr(), int(level.ndim == 3),
                                  *[t.data_ptr() if t is not None else 0 for t in (tl, th)], *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _ref_sep(fleet_a, fleet_b, lo, hi, k=None, **kw):
    """The pair entry on the gathered pairs, as (n, pairs, k)."""
    n, m_a, m_b, _ = _sizes(fleet_a, fleet_b)
    a, b, rl, rh = ci.gathered(fleet_a, fleet_b, lo, hi)
    return [x.reshape(n, m_a * m_b, -1) if x is not None else None for x in sg._sep(a, b, rl, rh, None, k=k, **kw)]


def _ref_con(fleet_a, fleet_b, level, lo, hi, **kw):
    n, m_a, m_b, _ = _sizes(fleet_a, fleet_b)
    a, b, rl, rh = ci.gathered(fleet_a, fleet_b, lo, hi)
    return [x.reshape(n, m_a * m_b, -1) if x is not None else None for x in cg._con(a, b, ci.wide_level(level, m_a * m_b), rl, rh, None, **kw)]


def _shares(want, what):
    """The conditions on the inputs, on the pair entry's outputs alone: at least 25 % of the times finite and at least 10 % NaN."""
    finite, missing = float(np.isfinite(want[0]).mean()), float(np.isnan(want[0]).mean())
    assert finite >= 0.25 and missing >= 0.10, (what, finite, missing)
    assert np.array_equal(np.isnan(want[0]), np.isnan(want[1])), what
    return finite


def _scenes(fleet, rows):
    return [[np.ascontiguousarray(x[rows]) for x in axis] for axis in fleet]


def _vehicles(fleet, order):
    return [[np.ascontiguousarray(x[:, order]) for x in axis] for axis in fleet]


def _copy(fleet):
    return [[x.copy() for x in axis] for axis in fleet]


# ---------------------------------------------------------------- 1. forward; 2. NULL arguments; 3. the NaN rule
def test_forward_is_the_pair_entry_bit_for_bit(shape, d):
    m_a, m_b, n, ks, _ = SHAPES[shape]
    d = int(d)      # one number of axes per process: a case stays at a few seconds
    pairs = m_a * m_b
    fleet_a, fleet_b = ci.fleets(n, m_a, m_b, d)
    for k in ks:
        lo, hi = ci.scene_windows(fleet_a, fleet_b, k, 900 + k)
        want = _ref_sep(fleet_a, fleet_b, lo, hi)
        got = _vs(fleet_a, fleet_b, lo, hi)
        assert _all_same(got, want), (shape, d, k)
        print("%s d = %d k = %d: %d queries the same bits in value and time; %.1f %% finite" % (shape, d, k, want[0].size, 100 * np.isfinite(want[0]).mean()))
        both = dict(zip(LAYOUTS, ci.levels_of(fleet_a, fleet_b, lo, hi, ci.level_seed(shape, d, k))))
        reached = {}
        for layout, level in both.items():
            want_c = _ref_con(fleet_a, fleet_b, level, lo, hi)
            reached[layout] = _icp(fleet_a, fleet_b, level, lo, hi)
            finite = _shares(want_c, (shape, d, k, layout))
            assert _all_same(reached[layout], want_c), (shape, d, k, layout)
            print("%s d = %d k = %d, level %s: %d queries the same bits in time and rate; %.1f %% finite"
                  % (shape, d, k, layout, want_c[0].size, 100 * finite))
        if shape != "3x5x20" or k != 7:
            continue
        # ---- NULL arguments: a NULL window end is the infinite one, bit for bit, and the pair entry's
        inf = np.full(lo.shape, np.inf)
        assert _all_same(_vs(fleet_a, fleet_b, None, hi), _vs(fleet_a, fleet_b, -inf, hi)) and _all_same(_vs(fleet_a, fleet_b, lo, None), _vs(fleet_a, fleet_b, lo, inf))
        assert _all_same(_vs(fleet_a, fleet_b, None, None, k=k), _vs(fleet_a, fleet_b, -inf, inf))
        assert _all_same(_vs(fleet_a, fleet_b, None, None, k=k), _ref_sep(fleet_a, fleet_b, None, None, k=k))
        for f in range(2):      # each output alone: the same bits, nothing else written (the sentinels behind every output: Out.get)
            some = _vs(fleet_a, fleet_b, lo, hi, want=[w == f for w in range(2)])
            assert some[1 - f] is None and _same_bits(some[f], got[f]), (d, f)
        still_a, still_b = _copy(fleet_a), _copy(fleet_b)      # NULL end velocities are zeros
        for axis in still_a + still_b:
            axis[3][:], axis[4][:] = 0.0, 0.0
        assert _all_same(_vs(still_a, still_b, lo, hi, zero_vel=True), _vs(still_a, still_b, lo, hi))
        assert _all_same(_vs(still_a, still_b, lo, hi, zero_vel=True), _ref_sep(still_a, still_b, lo, hi))
        for layout, level in both.items():
            run = lambda *w, **kw: _icp(fleet_a, fleet_b, level, *w, **kw)      # noqa: E731
            assert _all_same(run(None, hi), run(-inf, hi)) and _all_same(run(lo, None), run(lo, inf)) and _all_same(run(None, None), run(-inf, inf))
            assert _all_same(run(None, None), _ref_con(fleet_a, fleet_b, level, None, None))
            alone = run(lo, hi, want_rate=False)
            assert alone[1] is None and _same_bits(alone[0], reached[layout][0]), (d, layout)
            assert _all_same(_icp(still_a, still_b, level, lo, hi, zero_vel=True), _icp(still_a, still_b, level, lo, hi))
            assert _all_same(_icp(still_a, still_b, level, lo, hi, zero_vel=True), _ref_con(still_a, still_b, level, lo, hi))
        # ---- the NaN rule: a duration of 0, -1, inf, NaN in one axis of one vehicle of A makes exactly its row of m_b pairs of that
        # scene NaN, in one vehicle of B exactly its column of m_a pairs, and changes no other bit
        i, j = ci.pairs_of(m_a, m_b)
        hit_a = ((3, 0, 0, 6, 0.0), (9, 2, d - 1, 7, -1.0), (17, 1, 0, 7, np.inf), (19, 1, d - 1, 6, np.nan))      # scene, vehicle, axis, field
        hit_b = ((2, 4, 0, 6, 0.0), (8, 0, d - 1, 7, -1.0), (12, 3, 0, 7, np.inf), (18, 2, d - 1, 6, np.nan))
        for side, hits in enumerate((hit_a, hit_b)):
            bad = [_copy(fleet_a), _copy(fleet_b)]
            poisoned = np.zeros(got[0].shape, dtype=bool)
            for s, v, c, f, value in hits:
                bad[side][c][f][s, v] = value
                poisoned[s, (j if side else i) == v, :] = True
            assert poisoned.sum() == len(hits) * (m_a if side else m_b) * k
            runs = [(_vs(bad[0], bad[1], lo, hi), got)] + [(_icp(bad[0], bad[1], both[layout], lo, hi), reached[layout]) for layout in LAYOUTS]
            for out, ref in runs:
                for x, y in zip(out, ref):
                    assert np.array_equal(np.isnan(x), poisoned | np.isnan(y)), (d, side)
                    assert np.array_equal(_bits(x[~poisoned]), _bits(y[~poisoned])), (d, side)
        # a NaN, +inf, negative or -inf per-scene level makes exactly that scene-query's pairs NaN, with the pair entry's bits
        spoilt = both["per scene"].copy()
        gone = np.zeros(got[0].shape, dtype=bool)
        for s, q, value in ((2, 0, np.nan), (11, 3, np.inf), (14, 6, -1.0), (19, 6, -np.inf)):
            spoilt[s, q] = value
            gone[s, :, q] = True
        out = _icp(fleet_a, fleet_b, spoilt, lo, hi)
        for x, y in zip(out, reached["per scene"]):
            assert np.array_equal(np.isnan(x), gone | np.isnan(y)), d
            assert np.array_equal(_bits(x[~gone]), _bits(y[~gone])), d
        assert _all_same(out, _ref_con(fleet_a, fleet_b, spoilt, lo, hi))
        print("%s d = %d k = %d: NULL arguments and the NaN rule, rows and columns of %d pairs" % (shape, d, k, pairs))


# ---------------------------------------------------------------- 4. pointwise
def test_bits_depend_on_the_scene_and_its_query_only():
    m_a, m_b, n, k = 3, 5, 20, 7
    for d in (1, 2, 3):
        fleet_a, fleet_b = ci.fleets(n, m_a, m_b, d)
        lo, hi = ci.scene_windows(fleet_a, fleet_b, k, 950 + d)
        levels = ci.levels_of(fleet_a, fleet_b, lo, hi, 300 + d)

        def both(fa, fb, lv, w_lo, w_hi):
            """the separation entry's two outputs, then the contact entry's two in each layout"""
            out = _vs(fa, fb, w_lo, w_hi)
            for level in lv:
                out = out + _icp(fa, fb, level, w_lo, w_hi)
            return out

        first = both(fleet_a, fleet_b, levels, lo, hi)
        assert np.isfinite(first[2]).mean() >= 0.25
        assert _all_same(first, both(fleet_a, fleet_b, levels, lo, hi)), "differs from run to run"
        order = np.random.default_rng(5).permutation(n)
        assert _all_same(both(_scenes(fleet_a, order), _scenes(fleet_b, order), [x[order] for x in levels], lo[order], hi[order]),
                         [x[order] for x in first]), d
        # the vehicles of B permuted: the columns permute and no bit changes (and the rows, with A's)
        for side, m in ((1, m_b), (0, m_a)):
            turn = np.random.default_rng(6 + side).permutation(m)
            square = lambda x: x.reshape(n, m_a, m_b, k)      # noqa: E731
            moved = (lambda x: square(x)[:, :, turn, :] if side else square(x)[:, turn, :, :])      # noqa: E731
            flat = lambda x: np.ascontiguousarray(moved(x).reshape(n, m_a * m_b, k))      # noqa: E731
            fa, fb = (fleet_a, _vehicles(fleet_b, turn)) if side else (_vehicles(fleet_a, turn), fleet_b)
            assert _all_same(both(fa, fb, [flat(levels[0]), levels[1]], lo, hi), [flat(x) for x in first]), (d, side)
        for rows in (slice(0, 1), slice(12, 13), slice(19, 20), slice(n - 9, n)):      # single scenes, and the last 9 as a batch of their own
            part = both(_scenes(fleet_a, rows), _scenes(fleet_b, rows), [np.ascontiguousarray(x[rows]) for x in levels], lo[rows], hi[rows])
            assert _all_same(part, [x[rows] for x in first]), (d, rows)
        for at in (0, 3, 7):      # the seven columns inside a launch of eight: every query lands in another thread, next to another query
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=x.ndim - 1))      # noqa: E731
            eight = both(fleet_a, fleet_b, [wide(x, 1.0) for x in levels], wide(lo, 0.1), wide(hi, 0.2))
            assert _all_same([np.delete(x, at, axis=2) for x in eight], first), (d, at)
    print("the same bits in any order of the scenes and of either fleet's vehicles, in any batch and in any launch shape, in both layouts")


# ---------------------------------------------------------------- 5. A is A
def test_a_is_a():
    """With the fleets exchanged the call is the pair entry with A and B exchanged, (n, m_b, m_a, k): on 3 x 5 that is caught by shape, so
    also on 3 x 3, with distinct fleets and per-pair levels that are not symmetric."""
    n, k = 20, 7
    for m_a, m_b in ((3, 5), (3, 3)):
        for d in (1, 2, 3):
            fleet_a, fleet_b = ci.fleets(n, m_a, m_b, d)
            lo, hi = ci.scene_windows(fleet_a, fleet_b, k, 980 + d)
            level = ci.levels_of(fleet_a, fleet_b, lo, hi, 300 + d)[0]
            turned = np.ascontiguousarray(level.reshape(n, m_a, m_b, k).transpose(0, 2, 1, 3).reshape(n, m_b * m_a, k))      # the level of (j, i)
            assert not np.array_equal(level, turned)
            there = _vs(fleet_a, fleet_b, lo, hi) + _icp(fleet_a, fleet_b, level, lo, hi)
            back = _vs(fleet_b, fleet_a, lo, hi) + _icp(fleet_b, fleet_a, turned, lo, hi)
            want = _ref_sep(fleet_b, fleet_a, lo, hi) + _ref_con(fleet_b, fleet_a, turned, lo, hi)
            assert _all_same(back, want), (m_a, m_b, d)
            # under permute, the distances are those of the call as it was (the squared distance does not know which vehicle is A)
            unturned = np.ascontiguousarray(back[0].reshape(n, m_b, m_a, k).transpose(0, 2, 1, 3).reshape(n, m_a * m_b, k))
            both_finite = np.isfinite(unturned) & np.isfinite(there[0])
            assert np.array_equal(np.isnan(unturned), np.isnan(there[0])) and np.allclose(unturned[both_finite], there[0][both_finite], rtol=1e-9, atol=1e-9)
            # the mistake the case is for: B's vehicles read as A's.  m_a = m_b: the shape cannot tell, the values do
            if m_a == m_b:
                assert not _all_same(there, back), (m_a, m_b, d)
    print("the fleets exchanged: the pair entry with A and B exchanged, on 3 x 5 and on 3 x 3")


# ---------------------------------------------------------------- 6. reverse mode; 7. forward mode
def _leaves(fleet):
    return fg._fleet_leaves(fleet)


def _run_sep(la, lb, lo, hi):
    return rp.trajectory_cross_separation([la[f] for f in SIX], [lb[f] for f in SIX], lo, hi)


def _run_con(la, lb, level, lo, hi, radius=None):
    return rp.trajectory_cross_contact([la[f] for f in SIX], [lb[f] for f in SIX], radius, lo, hi, level_sq=level)


def _expanded(la, lb):
    """the pair entry's leaves: A's eight and B's eight, (n pairs, d) each, detached so that each pair's terms stay apart"""
    n, m_a, d = la[0].shape
    m_b = lb[0].shape[1]
    i, j = (torch.as_tensor(x, device=la[0].device) for x in ci.pairs_of(m_a, m_b))
    wide = lambda t, which: t.detach()[:, which, :].reshape(-1, d).clone().requires_grad_()      # noqa: E731
    return [wide(t, i) for t in la], [wide(t, j) for t in lb]


def _rep(w, pairs, leaf=False):
    if w is None:
        return None
    out = w.detach().unsqueeze(1).expand(w.shape[0], pairs, w.shape[1]).reshape(-1, w.shape[1]).contiguous()
    return out.clone().requires_grad_() if leaf else out


def _wide_level(level, pairs):
    k = level.shape[-1]
    return level.reshape(-1, k) if level.dim() == 3 else level.unsqueeze(1).expand(level.shape[0], pairs, k).reshape(-1, k)


def _fold(terms, shape, axis):
    """a pair's gradients, (n pairs, d), added into the vehicles of A (axis 2: over the partners of B) or B (axis 1), in longdouble"""
    n, m_a, m_b = shape
    return terms.reshape(n, m_a, m_b, -1).sum(axis=axis)


def _reference(out, leaves, extra, g, shape, fold_extra):
    """(the gradients of sum(g * out) in A's eight, B's eight and the `extra` leaves; the sums of the absolute values of their terms):
    the pair entry's own autograd, one backward per query column so that every (pair, query) term stays apart, the terms added in
    longdouble.  fold_extra(terms of an extra leaf as (n, pairs, k)) -> its gradient's shape."""
    n, m_a, m_b = shape
    k = out.shape[1]
    total, size = None, None
    for q in range(k):
        column = torch.zeros_like(out)
        column[:, q] = g.reshape(-1, k)[:, q]
        terms = [x.cpu().numpy().astype(LD) for x in torch.autograd.grad(out, leaves + extra, grad_outputs=column, retain_graph=True)]
        parts = [_fold(terms[f], shape, 2) for f in range(8)] + [_fold(terms[8 + f], shape, 1) for f in range(8)]
        sizes = [_fold(np.abs(terms[f]), shape, 2) for f in range(8)] + [_fold(np.abs(terms[8 + f]), shape, 1) for f in range(8)]
        parts += [fold_extra(x.reshape(n, m_a * m_b, k)) for x in terms[16:]]
        sizes += [fold_extra(np.abs(x).reshape(n, m_a * m_b, k)) for x in terms[16:]]
        total = parts if total is None else [x + y for x, y in zip(total, parts)]
        size = sizes if size is None else [x + y for x, y in zip(size, sizes)]
    return total, size


def _close(got, total, size, what):
    """fleet_gpu_cases._assert_close -- 1e-12 of the sum of |terms|, the eight gradients of one vehicle and axis sharing the largest of
    their eight sums -- for A's eight with the other leaves behind them, and for B's eight"""
    worst = fg._assert_close(got[:8] + got[16:], total[:8] + total[16:], size[:8] + size[16:], what + ", fleet A and the queries")
    return max(worst, fg._assert_close(got[8:16], total[8:16], size[8:16], what + ", fleet B"))


def _duality(g, got_dot, ref_dot, got, dots):
    """(reverse against forward mode, forward mode against the pair entry's): of the sum of |terms|"""
    gn, dn = g.cpu().numpy(), [t.cpu().numpy() for t in dots]
    left_terms = [np.where(np.isnan(got_dot), 0, gn.astype(LD) * got_dot)]
    right_terms = [x.astype(LD) * t for x, t in zip(got, dn)]
    left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
    scale = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
    ref_left = float(np.where(np.isnan(ref_dot), 0, gn.astype(LD) * ref_dot).sum())
    assert np.array_equal(np.isnan(ref_dot), np.isnan(got_dot))
    return abs(left - right) / scale, abs(left - ref_left) / scale


def _raises_on_double_backward(value, leaf):
    (g0,) = torch.autograd.grad((torch.nan_to_num(value) ** 2).sum(), leaf, create_graph=True)
    try:
        g0.sum().backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("double backward did not raise")


def test_autograd_against_the_pair_entry(d):
    d = int(d)
    m_a, m_b, n, k = 3, 5, 20, 7
    pairs, shape = m_a * m_b, (n, m_a, m_b)
    fleet_a, fleet_b = ci.fleets(n, m_a, m_b, d)
    lo_np, hi_np = ci.scene_windows(fleet_a, fleet_b, k, 960 + d)
    rng = np.random.default_rng(961)
    g = _t(rng.standard_normal((n, pairs, k)))
    gather = lambda ts, which: [t[:, which, :].reshape(-1, d) for t in ts]      # noqa: E731
    i, j = (torch.as_tensor(x, device=g.device) for x in ci.pairs_of(m_a, m_b))
    per_scene = lambda x: x.sum(axis=1)      # noqa: E731

    # ---- the separation: all sixteen fleet tensors, lo and hi
    la, lb = _leaves(fleet_a), _leaves(fleet_b)
    lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
    outs = _run_sep(la, lb, lo, hi)
    assert len(outs) == 2 and outs[0].shape == (n, pairs, k) and outs[0].requires_grad and not outs[1].requires_grad
    every = la + lb + [lo, hi]
    ea, eb = _expanded(la, lb)
    lo_e, hi_e = _rep(lo, pairs, leaf=True), _rep(hi, pairs, leaf=True)
    ref = rp.trajectory_separation([ea[f] for f in SIX], [eb[f] for f in SIX], lo_e, hi_e, None)
    assert _same_bits(outs[0].detach().cpu().numpy().reshape(-1, k), ref[0].detach().cpu().numpy())
    assert _same_bits(outs[1].cpu().numpy().reshape(-1, k), ref[1].cpu().numpy())
    total, size = _reference(ref[0], ea + eb, [lo_e, hi_e], g, shape, per_scene)
    got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    again = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
    assert all(np.isfinite(x).all() for x in got) and any(np.any(x != 0) for x in got[16:])
    worst = _close(got, total, size, "separation, reverse mode")
    print("d = %d: separation, reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, asserted 1e-12"
          % (d, worst))
    miss = torch.isnan(outs[0].detach())
    assert int(miss.sum()) > 0      # a NaN value has gradient exactly 0
    for x in torch.autograd.grad(outs[0], every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
        assert float(x.abs().max()) == 0.0
    dots = [_t(rng.standard_normal((n, m_a, d))) for _ in range(8)] + [_t(rng.standard_normal((n, m_b, d))) for _ in range(8)]
    dots += [_t(rng.standard_normal((n, k))) for _ in range(2)]
    with fwAD.dual_level():
        dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
        douts = _run_sep(dual[:8], dual[8:16], dual[16], dual[17])
        got_dot = fwAD.unpack_dual(douts[0]).tangent.cpu().numpy()
        assert fwAD.unpack_dual(douts[1]).tangent is None
        pa, pb = gather(dual[:8], i), gather(dual[8:16], j)
        wide = lambda w: w.unsqueeze(1).expand(n, pairs, k).reshape(-1, k)      # noqa: E731
        ref_dot = fwAD.unpack_dual(rp.trajectory_separation([pa[f] for f in SIX], [pb[f] for f in SIX], wide(dual[16]), wide(dual[17]), None)[0]).tangent
        ref_dot = ref_dot.cpu().numpy().reshape(got_dot.shape)
    _, func_dot = torch.func.jvp(lambda *xs: _run_sep(list(xs[:8]), list(xs[8:16]), xs[16], xs[17])[0], tuple(x.detach() for x in every), tuple(dots))
    assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
    dual_err, ref_err = _duality(g, got_dot, ref_dot, got, dots)
    print("d = %d: separation, duality between the modes %.2e of the sum of |terms|; forward mode against the pair entry's %.2e" % (d, dual_err, ref_err))
    assert dual_err <= 1e-12 and ref_err <= 1e-12
    _raises_on_double_backward(_run_sep(la, lb, lo, hi)[0], la[1])

    # ---- the contact, in both layouts of the level: all sixteen fleet tensors and the level; no gradient for lo and hi
    for layout, level_np in zip(LAYOUTS, ci.levels_of(fleet_a, fleet_b, lo_np, hi_np, 300 + d)):
        la, lb = _leaves(fleet_a), _leaves(fleet_b)
        if layout == "per pair":      # the whole row of one vehicle of A out of reach: a negative level is never reached
            level_np = level_np.copy()
            level_np.reshape(n, m_a, m_b, k)[4, 1] = -1.0
        level = _t(level_np).requires_grad_()
        fold_level = (lambda x: x) if layout == "per pair" else per_scene
        out = _run_con(la, lb, level, lo, hi)
        assert isinstance(out, torch.Tensor) and out.shape == (n, pairs, k) and out.requires_grad
        every = la + lb + [level]
        ea, eb = _expanded(la, lb)
        level_e = _wide_level(level.detach(), pairs).clone().requires_grad_()
        ref = rp.trajectory_contact([ea[f] for f in SIX], [eb[f] for f in SIX], None, _rep(lo, pairs), _rep(hi, pairs), None, level_sq=level_e)
        assert _same_bits(out.detach().cpu().numpy().reshape(-1, k), ref.detach().cpu().numpy())
        miss = torch.isnan(out.detach())
        share = float(miss.double().mean())
        assert 0.10 <= share <= 0.75, share      # the conditions on the inputs, on the pair entry's times
        total, size = _reference(ref, ea + eb, [level_e], g, shape, fold_level)
        grads = torch.autograd.grad(out, every + [lo, hi], grad_outputs=g, retain_graph=True, allow_unused=True)
        assert all(x is None or float(x.abs().max()) == 0.0 for x in grads[17:]), "a window end has a gradient"
        got = [x.cpu().numpy() for x in grads[:17]]
        again = [x.cpu().numpy() for x in torch.autograd.grad(out, every, grad_outputs=g, retain_graph=True)]
        assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
        assert all(np.isfinite(x).all() for x in got) and got[16].shape == level_np.shape
        worst = _close(got, total, size, "contact, reverse mode, level %s" % layout)
        print("d = %d, level %s: contact, reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, "
              "asserted 1e-12; %.1f %% of the levels unreached" % (d, layout, worst, 100 * share))
        if layout == "per pair":      # the vehicle whose whole row is unreached: exactly 0 in all eight tensors, all others finite (above)
            assert bool(miss.reshape(n, m_a, m_b, k)[4, 1].all())
            assert all(np.all(x[4, 1] == 0.0) for x in got[:8]) and any(np.any(x[4, 0] != 0.0) for x in got[:8])
        for x in torch.autograd.grad(out, every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
            assert float(x.abs().max()) == 0.0      # an unreached level has gradient exactly 0
        dots = [_t(rng.standard_normal((n, m_a, d))) for _ in range(8)] + [_t(rng.standard_normal((n, m_b, d))) for _ in range(8)]
        dots += [_t(rng.standard_normal(level_np.shape))]
        with fwAD.dual_level():
            dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
            got_dot = fwAD.unpack_dual(_run_con(dual[:8], dual[8:16], dual[16], lo.detach(), hi.detach())).tangent.cpu().numpy()
            pa, pb = gather(dual[:8], i), gather(dual[8:16], j)
            ref_dual = rp.trajectory_contact([pa[f] for f in SIX], [pb[f] for f in SIX], None, _rep(lo, pairs), _rep(hi, pairs), None,
                                             level_sq=_wide_level(dual[16], pairs))
            ref_dot = fwAD.unpack_dual(ref_dual).tangent.cpu().numpy().reshape(got_dot.shape)
        _, func_dot = torch.func.jvp(lambda *xs: _run_con(list(xs[:8]), list(xs[8:16]), xs[16], lo.detach(), hi.detach()),
                                     tuple(x.detach() for x in every), tuple(dots))
        assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
        dual_err, ref_err = _duality(g, got_dot, ref_dot, got, dots)
        print("d = %d, level %s: contact, duality between the modes %.2e of the sum of |terms|; forward mode against the pair entry's %.2e"
              % (d, layout, dual_err, ref_err))
        assert dual_err <= 1e-12 and ref_err <= 1e-12
        _raises_on_double_backward(_run_con(la, lb, level, lo, hi), la[1])

    # ---- a (n, m_a, m_b, k) radius built from a radius per vehicle: their gradients by the chain rule through the sum, the expand and
    # radius * radius, against the pair entry's given the radius per pair
    la, lb = _leaves(fleet_a), _leaves(fleet_b)
    r_a, r_b = _t(rng.uniform(1.0, 3.0, (n, m_a))).requires_grad_(), _t(rng.uniform(1.0, 3.0, (n, m_b))).requires_grad_()
    radius = (r_a[:, :, None, None] + r_b[:, None, :, None]).expand(n, m_a, m_b, k)
    out = _run_con(la, lb, None, lo, hi, radius=radius)
    ea, eb = _expanded(la, lb)
    radius_e = radius.detach().reshape(-1, k).clone().requires_grad_()
    ref = rp.trajectory_contact([ea[f] for f in SIX], [eb[f] for f in SIX], radius_e, _rep(lo, pairs), _rep(hi, pairs), None)
    assert out.shape == (n, pairs, k) and _same_bits(out.detach().cpu().numpy().reshape(-1, k), ref.detach().cpu().numpy())
    finite = float(torch.isfinite(out.detach()).double().mean())
    assert finite >= 0.05, finite
    total, size = _reference(ref, ea + eb, [radius_e], g, shape, lambda x: x)
    square = lambda x: x.reshape(n, m_a, m_b, k)      # noqa: E731
    total = total[:16] + [square(total[16]).sum(axis=(2, 3)), square(total[16]).sum(axis=(1, 3))]
    size = size[:16] + [square(size[16]).sum(axis=(2, 3)), square(size[16]).sum(axis=(1, 3))]
    got = [x.cpu().numpy() for x in torch.autograd.grad(out, la + lb + [r_a, r_b], grad_outputs=g)]
    assert got[16].shape == (n, m_a) and got[17].shape == (n, m_b) and all(np.isfinite(x).all() for x in got)
    worst = _close(got, total, size, "contact, reverse mode, a radius per vehicle")
    print("d = %d: a radius per vehicle as (n, m_a, m_b, k): at most %.2e of the sum of |terms|, asserted 1e-12; %.1f %% finite" % (d, worst, 100 * finite))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 8. obstacles
def test_obstacles():
    """static_fleet of 4 points against a fleet of 3 in d = 2: sep_sq, its time and the contact time are the pair entries' bits with the
    static spline as B; the gradient in the points is finite and the pair entry's through the same static_fleet composition, to 1e-12 of
    the sum of |terms|."""
    n, m_a, m_b, d, k = 20, 3, 4, 2, 7
    pairs, shape = m_a * m_b, (n, m_a, m_b)
    fleet_a, _ = ci.fleets(n, m_a, 1, d)
    la = _leaves(fleet_a)
    rng = np.random.default_rng(34)
    points = _t(rng.uniform(-5, 5, (n, m_b, d))).requires_grad_()
    duration = 2.5      # covers some of the vehicles' total times and not others: the common domain ends at the smaller
    six_a = [la[f] for f in SIX]
    obstacles = rp.static_fleet(points, duration)
    totals = np.min([axis[6] + axis[7] for axis in fleet_a], axis=0).min(axis=1)      # (n,): the scene's shortest vehicle
    lo_np = np.sort(rng.uniform(-0.1, 1.1, (n, k, 2)), axis=2) * np.minimum(totals, duration)[:, None, None]
    lo_np[:, :2, 0], lo_np[:, :2, 1] = -np.inf, np.inf
    lo, hi = _t(np.ascontiguousarray(lo_np[:, :, 0])), _t(np.ascontiguousarray(lo_np[:, :, 1]))
    outs = rp.trajectory_cross_separation(six_a, obstacles, lo, hi)
    # the pair entry on the gathered pairs, through the same composition: expanded points, then static_fleet
    i, j = (torch.as_tensor(x, device=points.device) for x in ci.pairs_of(m_a, m_b))
    ea = [t.detach()[:, i, :].reshape(-1, d).clone().requires_grad_() for t in la]
    points_e = points.detach()[:, j, :].reshape(-1, 1, d).clone().requires_grad_()
    eb = [t.reshape(-1, d) for t in rp.static_fleet(points_e, duration)]
    ref = rp.trajectory_separation([ea[f] for f in SIX], eb, _rep(lo, pairs), _rep(hi, pairs), None)
    assert _same_bits(outs[0].detach().cpu().numpy().reshape(-1, k), ref[0].detach().cpu().numpy())
    assert _same_bits(outs[1].cpu().numpy().reshape(-1, k), ref[1].cpu().numpy())
    value = outs[0].detach().cpu().numpy()
    assert np.isfinite(value).mean() >= 0.9 and (outs[1].cpu().numpy()[np.isfinite(value)] <= duration).all()
    g = _t(rng.standard_normal((n, pairs, k)))
    (got,) = torch.autograd.grad(outs[0], points, grad_outputs=g, retain_graph=True)
    (again,) = torch.autograd.grad(outs[0], points, grad_outputs=g, retain_graph=True)
    assert torch.isfinite(got).all() and torch.equal(got, again) and bool((got != 0).any())
    total, size = np.zeros((n, m_b, d), dtype=LD), np.zeros((n, m_b, d), dtype=LD)
    for q in range(k):
        column = torch.zeros_like(ref[0])
        column[:, q] = g.reshape(-1, k)[:, q]
        (terms,) = torch.autograd.grad(ref[0], points_e, grad_outputs=column, retain_graph=True)
        terms = terms.cpu().numpy().astype(LD).reshape(n, m_a, m_b, d)
        total += terms.sum(axis=1)
        size += np.abs(terms).sum(axis=1)
    err = np.abs(got.cpu().numpy().astype(LD) - total)
    worst = float(np.max(np.where(size > 0, err / np.where(size > 0, size, 1), 0)))
    print("d sep_sq / d points against the pair entry through the same composition: at most %.2e of the sum of |terms|, asserted 1e-12" % worst)
    assert np.all(err <= 1e-12 * size)
    # keep-out spheres: a radius per obstacle and vehicle; the contact times are the pair entry's, and fleet_first_contact's index is
    # into cross_pairs
    r_a, r_b = _t(rng.uniform(0.5, 1.5, (n, m_a))), _t(rng.uniform(1.0, 3.0, (n, m_b)))
    radius = (r_a[:, :, None, None] + r_b[:, None, :, None]).expand(n, m_a, m_b, k)
    t_contact = rp.trajectory_cross_contact(six_a, obstacles, radius, lo, hi)
    ref_t = rp.trajectory_contact([ea[f] for f in SIX], eb, radius.reshape(-1, k), _rep(lo, pairs), _rep(hi, pairs), None)
    assert _same_bits(t_contact.detach().cpu().numpy().reshape(-1, k), ref_t.detach().cpu().numpy())
    assert float(torch.isfinite(t_contact.detach()).double().mean()) >= 0.05
    t_first, pair = rp.fleet_first_contact(t_contact)
    table = rp.cross_pairs(m_a, m_b, device=pair.device)
    times = t_contact.detach().reshape(n, m_a, m_b, k)
    for s, q in zip(*torch.nonzero(pair >= 0, as_tuple=True)):
        vehicle, obstacle = table[:, pair[s, q]]
        assert times[s, vehicle, obstacle, q] == t_first[s, q]
    (g_points,) = torch.autograd.grad(torch.nan_to_num(t_first).sum(), points)
    assert torch.isfinite(g_points).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9. through the solves
def test_the_pipeline_is_the_composition():
    """min_time_cross_separation and min_time_cross_contact (m_a = 2, m_b = 3, d = 2, n = 100, k = 8, synchronised) on golden problems:
    the bits of min_time_solve + synchronize_axes + the cross calls composed by hand, and a finite gradient in pos1 of both fleets.  The
    level of a pair and query is the midpoint between the pair's least squared distance over the window and its squared distance at lo
    (section 27's case 4), one level per pair."""
    n, m_a, m_b, d, k = 100, 2, 3, 2, 8
    m, pairs = m_a + m_b, m_a * m_b
    pos = gg._golden_positions(n * m * d).reshape(n, m, d, 3)
    xa = [_t(np.ascontiguousarray(pos[:, :m_a, :, c])).requires_grad_() for c in range(3)]
    xb = [_t(np.ascontiguousarray(pos[:, m_a:, :, c])).requires_grad_() for c in range(3)]

    def spline_of(p):
        count = p[0].shape[1]
        sol = rp.min_time_solve(*[t.reshape(-1) for t in p], gap_tol=1e-13)
        six, _ = rp.synchronize_axes([t.reshape(n * count, d) for t in list(p) + [s.reshape(n, count, d) for s in sol[:3]]])
        return [t.reshape(n, count, d) for t in six], sol

    with torch.no_grad():
        six_a, _ = spline_of(xa)
        six_b, _ = spline_of(xb)
    st = [torch.cat([p, q], dim=1).detach().cpu().numpy() for p, q in zip(six_a, six_b)]
    good = np.isfinite(np.stack(st, 3)).all(axis=(1, 2, 3))
    z = np.zeros((n, m))
    whole = [[np.where(good[:, None], v, 1.0) for v in (st[0][..., c], st[1][..., c], st[2][..., c], z, z, st[3][..., c], st[4][..., c], st[5][..., c])]
             for c in range(d)]
    lo_np, hi_np = fg.scene_windows(whole, k, 970)
    lo, hi = _t(lo_np), _t(hi_np)
    i, j = ci.pairs_of(m_a, m_b)
    with torch.no_grad():
        least = rp.trajectory_cross_separation(six_a, six_b, lo, hi)[0]
        start = torch.zeros_like(least)
        for c in range(d):      # the window's start as it is: before 0 the cubics continue
            p = [rp.trajectory_eval(*[t[:, :, c].reshape(-1) for t in six], lo.unsqueeze(1).expand(n, six[0].shape[1], k).reshape(-1, k).contiguous())[0]
                 .reshape(n, -1, k) for six in (six_a, six_b)]
            start = start + (p[0][:, i, :] - p[1][:, j, :]) ** 2
    level = ((least + start) / 2).contiguous()      # one level per pair: with six pairs a scene's level is out of most pairs' reach
    sep = rp.min_time_cross_separation(xa, xb, lo, hi, gap_tol=1e-13)
    con = rp.min_time_cross_contact(xa, xb, None, lo, hi, level_sq=level, gap_tol=1e-13)
    assert len(sep) == 4 and len(con) == 3 and sep[0].shape == sep[1].shape == con[0].shape == (n, pairs, k)
    for sols, count in ((sep[2], m_a), (sep[3], m_b), (con[1], m_a), (con[2], m_b)):
        assert len(sols) == 5 and all(t.shape == (n, count, d) for t in sols)
    six_a, sol_a = spline_of(xa)
    six_b, sol_b = spline_of(xb)
    hand_sep = rp.trajectory_cross_separation(six_a, six_b, lo, hi)
    hand_con = rp.trajectory_cross_contact(six_a, six_b, None, lo, hi, level_sq=level)
    finite = torch.isfinite(hand_con.detach())
    print("%d of %d scenes solved finite, %.1f %% of the contact times finite" % (int(good.sum()), n, 100 * float(finite.double().mean())))
    assert good.mean() > 0.95 and float(finite.double().mean()) >= 0.25      # the condition, on the by-hand times
    same = lambda x, y: _same_bits(x.detach().cpu().numpy().astype(np.float64), y.detach().cpu().numpy().astype(np.float64))      # noqa: E731
    assert same(sep[0], hand_sep[0]) and same(sep[1], hand_sep[1]) and same(con[0], hand_con)
    for sols, sol, count in ((sep[2], sol_a, m_a), (sep[3], sol_b, m_b), (con[1], sol_a, m_a), (con[2], sol_b, m_b)):
        assert all(same(p, q.reshape(n, count, d)) for p, q in zip(sols, sol))
    ok = _t(good).bool()[:, None, None]
    g = _t(np.random.default_rng(971).uniform(0.5, 1.5, (n, pairs, k)))
    for out, mask in ((sep[0], torch.isfinite(sep[0].detach())), (con[0], finite)):
        grads = torch.autograd.grad(out, [xa[1], xb[1]], grad_outputs=torch.where(mask, g, torch.zeros_like(g)), retain_graph=True)
        by_hand = hand_sep[0] if out is sep[0] else hand_con
        hand_grads = torch.autograd.grad(by_hand, [xa[1], xb[1]], grad_outputs=torch.where(mask, g, torch.zeros_like(g)), retain_graph=True)
        for got, want in zip(grads, hand_grads):
            rows = ok.expand_as(got)
            assert torch.isfinite(got[rows]).all() and bool((got[rows] != 0).any()) and torch.equal(got[rows], want[rows])
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 10. beyond the grid's cap
def test_beyond_the_grid_cap(k):
    """m_a = 1, m_b = 3 in 100,001 scenes, 300,003 problems: more trips than the grid has blocks.  Both entries bit for bit the pair
    entries on the gathered pairs, at full size; no output element left at the sentinel; the scenes around problem 262,144, where the
    blocks start their second trip, equal the same scenes run alone.  The levels are grid_cap_gpu_cases' float64 stand-in."""
    import grid_cap_gpu_cases as gc
    k = int(k)
    m_a, m_b, n, d = 1, 3, gc.SCENES, 2
    pairs = m_a * m_b
    fleet_a, fleet_b = ci.fleets(n, m_a, m_b, d)
    lo, hi = ci.scene_windows(fleet_a, fleet_b, k, 900 + k)
    a, b, rl, rh = ci.gathered(fleet_a, fleet_b, lo, hi)
    per_pair = gc._plain_levels(a, b, rl, rh, np.zeros(rl.shape), 340 + k, squared=True).reshape(n, pairs, k)
    rows = gc.MID_SCENES
    full = _vs(fleet_a, fleet_b, lo, hi)
    gc._covered(full, ("cross separation", k))
    assert _all_same(full, [x.reshape(n, pairs, k) for x in sg._sep(a, b, rl, rh, None)]), (k, "the pair entry on the gathered pairs")
    assert _all_same(_vs(_scenes(fleet_a, rows), _scenes(fleet_b, rows), lo[rows], hi[rows]), [x[rows] for x in full]), (k, "the scenes alone")
    for layout, level in zip(LAYOUTS, (per_pair, ci.scene_levels(per_pair))):
        full = _icp(fleet_a, fleet_b, level, lo, hi)
        gc._covered(full, ("cross contact", layout, k))
        want = cg._con(a, b, ci.wide_level(level, pairs), rl, rh, None)
        assert _all_same(full, [x.reshape(n, pairs, k) for x in want]), (k, layout, "the pair entry on the gathered pairs")
        alone = _icp(_scenes(fleet_a, rows), _scenes(fleet_b, rows), np.ascontiguousarray(level[rows]), lo[rows], hi[rows])
        assert _all_same(alone, [x[rows] for x in full]), (k, layout, "the scenes alone")
        print("k = %d, level %s: %d problems the pair entry's bits; %.1f %% of the times finite" % (k, layout, n * pairs, 100 * np.isfinite(full[0]).mean()))


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
