"""The cases of tests/test_gpu_fleet_contact.py, each run in a fresh process (`python tests/fleet_contact_gpu_cases.py <case> [arguments]`),
on top of tests/fleet_gpu_cases.py's inputs and tests/contact_gpu_cases.py's pair entry.  Not collected by pytest (no test_ prefix on the
file).  What is checked, and why each bound is what it is: DESIGN.md section 27.  The reference throughout is the pair entry,
rp_trajectory_contact / trajectory_contact, on the pairs gathered in numpy or torch, with the scene's windows -- and a per-scene level --
repeated per pair and the delay NULL.  Per-pair levels are contact_ref.levels on the gathered pairs (seed 300 + d); the per-scene level of
scene s and query q is the per-pair level of pair (s + q) mod pairs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_gpu_cases as fg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import contact_gpu_cases as cg  # noqa: E402
import contact_ref as cf  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

LD = np.longdouble
SIX, SHAPES = fg.SIX, fg.SHAPES
_t, _bits, _same_bits, Out, _all_same = fg._t, fg._bits, fg._same_bits, fg.Out, fg.sg._all_same
fleet_inputs, scene_windows, pairs_of, gathered, _scenes = fg.fleet_inputs, fg.scene_windows, fg.pairs_of, fg.gathered, fg._scenes
LAYOUTS = ("per pair", "per scene")


def levels_of(fleet, lo, hi, seed):
    """(the per-pair levels (n, pairs, k), the per-scene levels (n, k)) of a fleet and its windows."""
    n, m = fleet[0][0].shape
    a, b, rl, rh = gathered(fleet, lo, hi)
    per_pair = cf.levels(a, b, rl, rh, np.zeros(rl.shape), seed)[0].reshape(n, m * (m - 1) // 2, -1)
    return per_pair, scene_levels(per_pair)


def scene_levels(per_pair):
    n, pairs, k = per_pair.shape
    pick = (np.arange(n)[:, None] + np.arange(k)[None, :]) % pairs
    return np.ascontiguousarray(np.take_along_axis(per_pair, pick[:, None, :], axis=1)[:, 0, :])


def _enc(fleet, level, lo, hi, want_rate=True, zero_vel=False):
    """The fleet entry: (time, rate), (n, pairs, k), rate None where not asked for.  A level of three dimensions goes in per pair, one of
    two per scene; lo / hi of None go in as NULL."""
    n, m = fleet[0][0].shape
    d, k = len(fleet), level.shape[-1]
    tf = [[_t(x) for x in axis] for axis in fleet]
    tv, tl, th = (_t(x) if x is not None else None for x in (level, lo, hi))
    outs = [Out(n, m * (m - 1) // 2, k), Out(n, m * (m - 1) // 2, k) if want_rate else None]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    capi.trajectory_fleet_contact(0, 0, n, m, k, d, addr, tv.data_ptr(), int(level.ndim == 3), *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                  *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _reference(fleet, level, lo, hi, **kw):
    """The pair entry on the gathered pairs, as (n, pairs, k)."""
    n, m = fleet[0][0].shape
    pairs = m * (m - 1) // 2
    a, b, rl, rh = gathered(fleet, lo, hi)
    wide = level.reshape(n * pairs, -1) if level.ndim == 3 else np.repeat(level, pairs, axis=0)
    return [x.reshape(n, pairs, -1) if x is not None else None for x in cg._con(a, b, np.ascontiguousarray(wide), rl, rh, None, **kw)]


def _shares(want, what):
    """The conditions on the inputs, on the pair entry's outputs alone: at least 25 % of the times finite and at least 10 % NaN."""
    finite = float(np.isfinite(want[0]).mean())
    missing = float(np.isnan(want[0]).mean())
    assert finite >= 0.25 and missing >= 0.10, (what, finite, missing)
    assert np.array_equal(np.isnan(want[0]), np.isnan(want[1])), what
    return finite


# ---------------------------------------------------------------- 1. forward
def test_forward_is_the_pair_entry_bit_for_bit(shape, d=None):
    m, n, ks, ds = SHAPES[shape]
    ds = ds if d is None else (int(d),)      # one number of axes per process: a case stays at a few seconds
    first, second = pairs_of(m)
    for d in ds:
        fleet = fleet_inputs(n, m, d)
        for k in ks:
            lo, hi = scene_windows(fleet, k, 900 + k)
            both = dict(zip(LAYOUTS, levels_of(fleet, lo, hi, 300 + d)))
            for layout, level in both.items():
                want = _reference(fleet, level, lo, hi)
                got = _enc(fleet, level, lo, hi)
                finite = _shares(want, (shape, d, k, layout))
                assert _all_same(got, want), (shape, d, k, layout)
                print("%s d = %d k = %d, level %s: %d queries the same bits in time and rate; %.1f %% finite" % (shape, d, k, layout, want[0].size, 100 * finite))
                if shape != "5x30" or k != 7:
                    continue
                # a NULL window end is the infinite one, bit for bit, and the pair entry's
                inf = np.full(lo.shape, np.inf)
                assert _all_same(_enc(fleet, level, None, hi), _enc(fleet, level, -inf, hi)) and _all_same(_enc(fleet, level, lo, None), _enc(fleet, level, lo, inf))
                assert _all_same(_enc(fleet, level, None, None), _enc(fleet, level, -inf, inf))
                assert _all_same(_enc(fleet, level, None, None), _reference(fleet, level, None, None))
                # no rate: the same times, nothing else written (the sentinels behind every output: Out.get)
                alone = _enc(fleet, level, lo, hi, want_rate=False)
                assert alone[1] is None and _same_bits(alone[0], got[0]), (d, layout)
                # NULL end velocities are zeros
                still = [[x.copy() for x in axis] for axis in fleet]
                for axis in still:
                    axis[3][:], axis[4][:] = 0.0, 0.0
                assert _all_same(_enc(still, level, lo, hi, zero_vel=True), _enc(still, level, lo, hi))
                assert _all_same(_enc(still, level, lo, hi, zero_vel=True), _reference(still, level, lo, hi))
                # the NaN rule: a duration of 0, -1, inf, NaN in one axis of one vehicle makes exactly that vehicle's m - 1 pairs of that
                # scene NaN and changes no other bit
                bad = [[x.copy() for x in axis] for axis in fleet]
                hit = ((3, 0, 0, 6, 0.0), (9, 4, d - 1, 7, -1.0), (17, 2, 0, 7, np.inf), (29, 1, d - 1, 6, np.nan))      # scene, vehicle, axis, field
                poisoned = np.zeros(got[0].shape, dtype=bool)
                for s, v, c, f, value in hit:
                    bad[c][f][s, v] = value
                    poisoned[s, (first == v) | (second == v), :] = True
                assert poisoned.sum() == len(hit) * (m - 1) * k
                for x, ref in zip(_enc(bad, level, lo, hi), got):
                    assert np.array_equal(np.isnan(x), poisoned | np.isnan(ref)), (d, layout)
                    assert np.array_equal(_bits(x[~poisoned]), _bits(ref[~poisoned])), (d, layout)
                if layout != "per scene":
                    continue
                # a NaN, +inf or negative per-scene level makes exactly that scene-query's pairs NaN and changes no other bit
                spoilt = level.copy()
                gone = np.zeros(got[0].shape, dtype=bool)
                for s, q, value in ((2, 0, np.nan), (11, 3, np.inf), (20, 6, -1.0), (29, 6, -np.inf)):
                    spoilt[s, q] = value
                    gone[s, :, q] = True
                for x, ref in zip(_enc(fleet, spoilt, lo, hi), got):
                    assert np.array_equal(np.isnan(x), gone | np.isnan(ref)), d
                    assert np.array_equal(_bits(x[~gone]), _bits(ref[~gone])), d
                assert _all_same(_enc(fleet, spoilt, lo, hi), _reference(fleet, spoilt, lo, hi))


# ---------------------------------------------------------------- 2. reproducibility
def test_bits_depend_on_the_scene_and_its_query_only():
    m, n, k = 5, 30, 7
    for d in (1, 2, 3):
        fleet = fleet_inputs(n, m, d)
        lo, hi = scene_windows(fleet, k, 950 + d)
        for layout, level in zip(LAYOUTS, levels_of(fleet, lo, hi, 300 + d)):
            first = _enc(fleet, level, lo, hi)
            assert np.isfinite(first[0]).mean() >= 0.25
            assert _all_same(first, _enc(fleet, level, lo, hi)), "differs from run to run"
            order = np.random.default_rng(5).permutation(n)
            assert _all_same(_enc(_scenes(fleet, order), level[order], lo[order], hi[order]), [x[order] for x in first]), (d, layout)
            for rows in (slice(0, 1), slice(12, 13), slice(29, 30), slice(n - 13, n)):      # single scenes, and the last 13 as a batch of their own
                part = _enc(_scenes(fleet, rows), np.ascontiguousarray(level[rows]), lo[rows], hi[rows])
                assert _all_same(part, [x[rows] for x in first]), (d, layout, rows)
            for at in (0, 3, 7):      # the seven columns inside a launch of eight: every query lands in another thread, next to another query
                wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=x.ndim - 1))      # noqa: E731
                eight = _enc(fleet, wide(level, 1.0), wide(lo, 0.1), wide(hi, 0.2))
                assert _all_same([np.delete(x, at, axis=2) for x in eight], first), (d, layout, at)
    print("the same bits in any order of the scenes, in any batch and in any launch shape, in both layouts of the level")


# ---------------------------------------------------------------- 3. autograd
def _run(leaves, level, lo, hi, radius=None):
    return rp.trajectory_fleet_contact([leaves[f] for f in SIX], radius, lo, hi, level_sq=level)


def _wide_level(level, pairs):
    """a level, per pair or per scene, as the pair entry's (n pairs, k)"""
    k = level.shape[-1]
    return level.reshape(-1, k) if level.dim() == 3 else level.unsqueeze(1).expand(level.shape[0], pairs, k).reshape(-1, k)


def _pairwise(splines, level, lo, hi, m, radius=False):
    """trajectory_contact on the pairs gathered in torch from eight (n, m, d) tensors: (the expanded leaves A (8), B (8) and the level or
    radius -- detached, so that each pair's terms stay apart -- and the times, (n pairs, k))"""
    n, _, d = splines[0].shape
    first, second = (torch.as_tensor(x, device=splines[0].device) for x in pairs_of(m))
    wide = lambda t, which: t.detach()[:, which, :].reshape(-1, d).clone().requires_grad_()      # noqa: E731
    a, b = [wide(t, first) for t in splines], [wide(t, second) for t in splines]
    rep = lambda w: w.detach().unsqueeze(1).expand(n, len(first), w.shape[1]).reshape(-1, w.shape[1]).contiguous() if w is not None else None      # noqa: E731
    level_e = _wide_level(level.detach(), len(first)).clone().requires_grad_()
    out = rp.trajectory_contact([a[f] for f in SIX], [b[f] for f in SIX], level_e if radius else None, rep(lo), rep(hi), None,
                                level_sq=None if radius else level_e)
    return a, b, level_e, out


def _reference_gradients(splines, level, lo, hi, m, g, radius=False):
    """(the gradients of sum(g * t_contact) in the eight (n, m, d) tensors and the level -- or the radius --; the sum of the absolute
    values of their terms; the pair entry's times): the pair entry's own autograd on the gathered pairs, one backward per query column so
    that every (pair, query) term stays apart, the terms added in longdouble."""
    n, _, d = splines[0].shape
    k = level.shape[-1]
    pairs = m * (m - 1) // 2
    a, b, level_e, out = _pairwise(splines, level, lo, hi, m, radius)
    leaves = a + b + [level_e]
    shape = (n, pairs, k) if level.dim() == 3 else (n, k)
    total = [np.zeros((n, m, d), dtype=LD) for _ in range(8)] + [np.zeros(shape, dtype=LD)]
    size = [np.zeros_like(x) for x in total]
    for q in range(k):
        column = torch.zeros_like(out)
        column[:, q] = g.reshape(-1, k)[:, q]
        terms = [x.cpu().numpy().astype(LD) for x in torch.autograd.grad(out, leaves, grad_outputs=column, retain_graph=True)]
        for f in range(8):
            total[f] += fg._folded(terms[f], terms[8 + f], n, m)
            size[f] += fg._folded(np.abs(terms[f]), np.abs(terms[8 + f]), n, m)
        share = terms[16].reshape(n, pairs, k)
        total[8] += share if level.dim() == 3 else share.sum(axis=1)
        size[8] += np.abs(share) if level.dim() == 3 else np.abs(share).sum(axis=1)
    return total, size, out


def test_autograd_against_the_pair_entry(d):
    d = int(d)
    m, n, k = 5, 30, 7
    pairs = m * (m - 1) // 2
    fleet = fleet_inputs(n, m, d)
    lo_np, hi_np = scene_windows(fleet, k, 960 + d)
    rng = np.random.default_rng(961)
    g = _t(rng.standard_normal((n, pairs, k)))
    for layout, level_np in zip(LAYOUTS, levels_of(fleet, lo_np, hi_np, 300 + d)):
        leaves = fg._fleet_leaves(fleet)
        lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
        level = _t(level_np).requires_grad_()
        out = _run(leaves, level, lo, hi)
        assert isinstance(out, torch.Tensor) and out.shape == (n, pairs, k) and out.requires_grad
        every = leaves + [level]
        total, size, ref_out = _reference_gradients(leaves, level, lo, hi, m, g)
        assert _same_bits(out.detach().cpu().numpy().reshape(-1, k), ref_out.detach().cpu().numpy())
        miss = torch.isnan(out.detach())
        share = float(miss.double().mean())
        assert 0.10 <= share <= 0.75, share      # the conditions on the inputs, on the pair entry's times
        grads = torch.autograd.grad(out, every + [lo, hi], grad_outputs=g, retain_graph=True, allow_unused=True)
        assert all(x is None or float(x.abs().max()) == 0.0 for x in grads[9:]), "a window end has a gradient"
        got = [x.cpu().numpy() for x in grads[:9]]
        again = [x.cpu().numpy() for x in torch.autograd.grad(out, every, grad_outputs=g, retain_graph=True)]
        assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
        assert all(np.isfinite(x).all() for x in got)
        assert got[8].shape == level_np.shape
        worst = fg._assert_close(got, total, size, "reverse mode, level %s" % layout)
        print("d = %d, level %s: reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, asserted "
              "1e-12; %.1f %% of the levels unreached" % (d, layout, worst, 100 * share))
        # an unreached level has gradient exactly 0 (the others, above, are all finite)
        for x in torch.autograd.grad(out, every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
            assert float(x.abs().max()) == 0.0
        # the radius: its gradient by the chain rule through radius * radius, against the pair entry's given the radius per pair
        radius = _t(np.sqrt(np.abs(level_np)) + 0.125).requires_grad_()
        by_radius = _run(leaves, None, lo, hi, radius=radius)
        r_total, r_size, r_out = _reference_gradients(leaves, radius, lo, hi, m, g, radius=True)
        assert _same_bits(by_radius.detach().cpu().numpy().reshape(-1, k), r_out.detach().cpu().numpy())
        assert 0.05 <= float(torch.isfinite(by_radius.detach()).double().mean())
        r_got = [x.cpu().numpy() for x in torch.autograd.grad(by_radius, every[:8] + [radius], grad_outputs=g)]
        assert r_got[8].shape == level_np.shape
        worst = fg._assert_close(r_got, r_total, r_size, "reverse mode, radius %s" % layout)
        print("d = %d, radius %s: at most %.2e of the sum of |terms|, asserted 1e-12; %.1f %% finite"
              % (d, layout, worst, 100 * float(torch.isfinite(by_radius.detach()).double().mean())))
        # forward mode, torch.func.jvp, duality
        dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal(level_np.shape))]
        with fwAD.dual_level():
            dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
            got_dot = fwAD.unpack_dual(_run(dual[:8], dual[8], lo.detach(), hi.detach())).tangent.cpu().numpy()
        _, func_dot = torch.func.jvp(lambda *xs: _run(list(xs[:8]), xs[8], lo.detach(), hi.detach()), tuple(x.detach() for x in every), tuple(dots))
        assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
        # against the pair entry's forward mode on the gathered pairs: per query one term per input, the same terms
        first, second = (torch.as_tensor(x, device=g.device) for x in pairs_of(m))
        gather = lambda t, which: t[:, which, :].reshape(-1, d)      # noqa: E731
        rep = lambda w: w.detach().unsqueeze(1).expand(n, pairs, k).reshape(-1, k)      # noqa: E731
        with fwAD.dual_level():
            dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
            pa, pb = [gather(t, first) for t in dual[:8]], [gather(t, second) for t in dual[:8]]
            ref = rp.trajectory_contact([pa[f] for f in SIX], [pb[f] for f in SIX], None, rep(lo), rep(hi), None, level_sq=_wide_level(dual[8], pairs))
            ref_dot = fwAD.unpack_dual(ref).tangent.cpu().numpy().reshape(got_dot.shape)
        gn, dn = g.cpu().numpy(), [t.cpu().numpy() for t in dots]
        left_terms = [np.where(np.isnan(got_dot), 0, gn.astype(LD) * got_dot)]
        right_terms = [x.astype(LD) * t for x, t in zip(got, dn)]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        scale = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        ref_left = float(np.where(np.isnan(ref_dot), 0, gn.astype(LD) * ref_dot).sum())
        print("d = %d, level %s: duality between reverse and forward mode: %.2e of the sum of |terms|; forward mode against the pair entry's: %.2e"
              % (d, layout, abs(left - right) / scale, abs(left - ref_left) / scale))
        assert abs(left - right) <= 1e-12 * scale and abs(left - ref_left) <= 1e-12 * scale
        assert np.array_equal(np.isnan(ref_dot), np.isnan(got_dot))
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(_run(leaves, level, lo, hi)) ** 2).sum(), leaves[1], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
    if d != 2:
        torch.cuda.synchronize()
        return
    # section 26's two hand-made scenes of three vehicles.  The squared distance of pair (0, 1) shrinks until the window ends, with vehicle
    # 1 at t = 3 and with vehicle 0 at t = 2; that of pair (0, 2) grows from the start.  Levels from their distances: column 0 the least
    # squared distance itself (pair (0, 2): the window's start; for the others the level is within rounding of an extreme of f, where the
    # entry may give the touch, a later contact or NaN and the rate may be 0: the pair entry's bits, whatever they are, and no gradient);
    # column 1 the midpoint between it and the squared distance at the start (reached inside the window, where the rate is not 0) or,
    # where the two are one number, one less (never reached): the gradients
    hand = fg._hand_made_scene()
    hl = fg._fleet_leaves(hand)
    six = [hl[f].detach() for f in SIX[:6]]
    least = rp.trajectory_fleet_separation(six)[0].detach()      # (2, 3, 1)
    start = sum((hl[0][:, :, c][:, [0, 0, 1]] - hl[0][:, :, c][:, [1, 2, 2]]) ** 2 for c in range(2)).detach().unsqueeze(2)
    print("hand-made scenes: the least squared distances %s, at the start %s" % (least.cpu().numpy().ravel(), start.cpu().numpy().ravel()))
    assert bool((start >= least).all()) and bool((start[:, 0] > least[:, 0]).all()) and bool((start[:, 1] == least[:, 1]).all())
    middle = torch.where(start > least, (start + least) / 2, least - 1.0)
    touch = torch.cat([least, middle], dim=2).contiguous()
    with torch.no_grad():
        at_touch = _run(hl, touch, None, None).cpu().numpy()
        assert _same_bits(at_touch.reshape(-1, 2), _pairwise(hl, touch, None, None, 3)[3].detach().cpu().numpy())
    print("hand-made scenes: the times at the least distances %s" % at_touch[:, :, 0].ravel())
    assert np.array_equal(at_touch[:, 1, 0], np.zeros(2))      # pair (0, 2): the window's start, where the level equals the value
    level = middle.clone().requires_grad_()
    out = _run(hl, level, None, None)
    total, size, ref_out = _reference_gradients(hl, level, None, None, 3, torch.ones_like(out))
    assert _same_bits(out.detach().cpu().numpy().reshape(-1, 1), ref_out.detach().cpu().numpy())
    times = out.detach().cpu().numpy()[:, :, 0]
    print("hand-made scenes: the times at the midpoint levels %s" % times.ravel())
    assert np.isfinite(times[:, 0]).all() and np.isnan(times[:, 1]).all() and (times[:, 0] > 0).all()
    assert (times[:, 0] < np.array([3.0, 2.0])).all()      # before the window ends, with vehicle 1 and with vehicle 0
    got = [x.cpu().numpy() for x in torch.autograd.grad(out.sum(), hl + [level])]
    assert all(np.isfinite(x).all() for x in got)
    fg._assert_close(got, total, size, "hand-made scenes")
    assert (got[8][:, 0, 0] < 0).all() and (got[8][:, 1, 0] == 0).all()      # a larger level is reached earlier; an unreached one: nothing
    assert all(np.any(got[1][:, v, :] != 0) for v in (0, 1))      # both vehicles of pair (0, 1) move the time; vehicle 2, whose
    assert np.isnan(times[:, 2]).all() and all(np.all(x[:, 2, :] == 0) for x in got[:8])      # pairs make no contact, gets exactly 0
    # a (k,) radius, six tensors
    row = _t(np.array([990.0, 995.0])).requires_grad_()      # between the pair (0, 1)'s distances at the start and at the end
    o = rp.trajectory_fleet_contact(six, row)
    assert o.shape == (2, 3, 2)
    (g_row,) = torch.autograd.grad(torch.nan_to_num(o).sum(), row)
    assert g_row.shape == (2,) and torch.isfinite(g_row).all() and bool((g_row != 0).all())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. through the solves
def test_the_pipeline_is_the_composition():
    """min_time_fleet_contact (m = 3, d = 2, n = 100, k = 8, synchronised) on golden problems: the bits of min_time_solve + synchronize_axes +
    trajectory_fleet_contact composed by hand; its gradient in pos1 finite, and within 1e-12 of the sum of |terms| of the same composition
    with the pair entry on the gathered pairs, a term being one (pair, query)'s share of the gradient and the unit the largest such sum
    among the vehicle's axes (fleet_gpu_cases' reason: the stretch to the slowest axis couples them).  The per-scene level of scene s and
    query q is the midpoint between the least squared distance of pair (s + q) mod pairs over the window and its squared distance at lo,
    from trajectory_fleet_separation and the evaluator on the device's own solutions (the evaluator does not clamp: at a lo before 0 the
    first segments' cubics continue, so no level is the distance at t = 0 exactly, where vehicles that start from rest have a rate of 0).  fleet_first_contact of the result
    against numpy's nanmin and argmin over the pairs."""
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
    lo_np, hi_np = scene_windows(fleet_np, k, 970)
    lo, hi = _t(lo_np), _t(hi_np)
    first, second = pairs_of(m)
    with torch.no_grad():
        least = rp.trajectory_fleet_separation(six, lo, hi)[0]
        at = lo.unsqueeze(1).expand(n, m, k).reshape(n * m, k).contiguous()      # the window's start as it is: before 0 the cubics continue
        start = torch.zeros_like(least)
        for c in range(d):
            p = rp.trajectory_eval(*[t[:, :, c].reshape(n * m) for t in six], at)[0].reshape(n, m, k)
            start = start + (p[:, first, :] - p[:, second, :]) ** 2
    level = _t(scene_levels(((least + start) / 2).cpu().numpy()))
    out = rp.min_time_fleet_contact(x, None, lo, hi, level_sq=level, gap_tol=1e-13)
    assert len(out) == 2 and len(out[1]) == 5 and all(t.shape == (n, m, d) for t in out[1]) and out[0].shape == (n, pairs, k)
    six, sol = spline_of(x)
    by_hand = rp.trajectory_fleet_contact(six, None, lo, hi, level_sq=level)
    finite = torch.isfinite(by_hand.detach())
    print("%d of %d scenes solved finite, %.1f %% of the times finite" % (int(good.sum()), n, 100 * float(finite.double().mean())))
    assert good.mean() > 0.95 and float(finite.double().mean()) >= 0.25
    assert _same_bits(out[0].detach().cpu().numpy(), by_hand.detach().cpu().numpy())
    assert all(_same_bits(p.detach().cpu().numpy().astype(np.float64), q.detach().cpu().numpy().reshape(n, m, d).astype(np.float64)) for p, q in zip(out[1], sol))
    # the scene's first contact and its pair
    t_first, pair = rp.fleet_first_contact(out[0])
    times = out[0].detach().cpu().numpy()
    filled = np.where(np.isfinite(times), times, np.inf)
    any_finite = np.isfinite(times).any(axis=1)
    with np.errstate(all="ignore"):
        want_first = np.where(any_finite, filled.min(axis=1), np.nan)
    assert np.array_equal(t_first.detach().cpu().numpy(), want_first, equal_nan=True)
    assert np.array_equal(pair.cpu().numpy(), np.where(any_finite, filled.argmin(axis=1), -1))
    assert any_finite.mean() > 0.25
    g = _t(np.random.default_rng(971).uniform(0.5, 1.5, tuple(out[0].shape)))
    g = torch.where(finite, g, torch.zeros_like(g))
    (got,) = torch.autograd.grad(out[0], x[1], grad_outputs=g, retain_graph=True)
    ok = _t(good).bool()[:, None, None].expand_as(got)
    assert torch.isfinite(got[ok]).all()
    # the loss a planner reads first, through fleet_first_contact: the same bits in every run
    loss = lambda: torch.autograd.grad(torch.nan_to_num(rp.fleet_first_contact(out[0])[0]).sum(), x[1], retain_graph=True)[0]      # noqa: E731
    assert torch.equal(loss()[ok], loss()[ok]) and torch.isfinite(loss()[ok]).all()
    # the reference: the same composition, the pair entry on the gathered pairs; one backward per (pair, query) through the solve
    eight = six[:3] + [torch.zeros_like(six[0]), torch.zeros_like(six[0])] + six[3:]
    a, b, _, ref_out = _pairwise(eight, level, lo, hi, m)
    assert _same_bits(ref_out.detach().cpu().numpy().reshape(n, pairs, k), by_hand.detach().cpu().numpy())
    total, size = np.zeros((n, m, d), dtype=LD), np.zeros((n, m, d), dtype=LD)
    table = (0, 1, 2, 5, 6, 7)      # the six of synchronize_axes in the table's order
    g_flat = g.reshape(n * pairs, k)
    for q in range(k):
        column = torch.zeros_like(ref_out)
        column[:, q] = g_flat[:, q]
        terms = torch.autograd.grad(ref_out, [a[f] for f in table] + [b[f] for f in table], grad_outputs=column, retain_graph=True)
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
    rows = good[:, None, None] & np.ones((n, m, d), dtype=bool)
    size = np.repeat(size.max(axis=2, keepdims=True), d, axis=2)      # the stretch to the slowest axis couples a vehicle's axes: their largest
    err = np.abs(got.cpu().numpy().astype(LD) - total)
    worst = float(np.max(np.where(rows & (size > 0), err / np.where(size > 0, size, 1), 0)))
    print("d t_contact / d pos1 through the pipeline against the same composition with the pair entry: at most %.2e of the sum of |terms|, asserted 1e-12" % worst)
    assert np.all(err[rows] <= 1e-12 * size[rows])
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
