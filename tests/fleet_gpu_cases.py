"""The cases of tests/test_gpu_fleet.py, each run in a fresh process (`python tests/fleet_gpu_cases.py <case> [arguments]`), on top of
tests/separation_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound is
what it is: DESIGN.md section 26.  The reference throughout is the pair entry, rp_trajectory_separation / trajectory_separation, on the
pairs gathered in torch or numpy, with the scene's windows repeated per pair and the delay NULL."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import separation_gpu_cases as sg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import separation_ref as sr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

LD = np.longdouble
SIX = sg.SIX
_t, _bits, _same_bits, Out = sg._t, sg._bits, sg._same_bits, sg.Out
# (m, n): with 128 problems per trip, 5 x 30 is 300 pair-problems -- three trips, the last partial, scenes straddling the trip boundaries;
# 3 x 43 is 129 -- a trailing single problem, and with k = 7 903 queries, a single trailing query; 2 x 300 the degenerate fleet; 64 x 1
# 2,016 problems of one scene
SHAPES = {"5x30": (5, 30, (1, 7, 8), (1, 2, 3)), "3x43": (3, 43, (1, 7, 8), (1, 2, 3)), "2x300": (2, 300, (1, 7, 8), (1, 2, 3)),
          "64x1": (64, 1, (1,), (2,))}


def fleet_inputs(n, m, d):
    """The fleet as d lists (the axes) of eight (n, m) arrays in the table's order: vehicle v, axis c is random_states(n, 1 + c + 3 v)."""
    per = [[tr.random_states(n, 1 + c + 3 * v) for v in range(m)] for c in range(d)]
    return [[np.ascontiguousarray(np.stack([per[c][v][f] for v in range(m)], axis=1)) for f in range(8)] for c in range(d)]


def scene_windows(fleet, k, seed):
    """Section 18's windows over each scene's domain, [0, the smallest total time of its m d splines]: (lo, hi), (n, k)."""
    n, m = fleet[0][0].shape
    every = [[axis[f][:, v] for f in range(8)] for axis in fleet for v in range(m)]
    return sr.windows(every, every, np.zeros((n, k)), seed)


def pairs_of(m):
    first, second = np.triu_indices(m, 1)
    return first, second


def gathered(fleet, lo, hi):
    """The pair entry's inputs: vehicles A and B as lists of d splines of n pairs values, problem s pairs + p, and the windows repeated."""
    n, m = fleet[0][0].shape
    first, second = pairs_of(m)
    a = [[np.ascontiguousarray(x[:, first].reshape(-1)) for x in axis] for axis in fleet]
    b = [[np.ascontiguousarray(x[:, second].reshape(-1)) for x in axis] for axis in fleet]
    rep = lambda w: np.ascontiguousarray(np.repeat(w, len(first), axis=0)) if w is not None else None      # noqa: E731
    return a, b, rep(lo), rep(hi)


def _fleet(fleet, lo, hi, k=None, want=(True, True), zero_vel=False):
    """The fleet entry: (value, time), (n, pairs, k), None where not asked for.  lo / hi of None go in as NULL."""
    n, m = fleet[0][0].shape
    d = len(fleet)
    k = k if k is not None else next(x for x in (lo, hi) if x is not None).shape[1]
    tf = [[_t(x) for x in axis] for axis in fleet]
    tl, th = (_t(x) if x is not None else None for x in (lo, hi))
    outs = [Out(n, m * (m - 1) // 2, k) if w else None for w in want]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    capi.trajectory_fleet_separation(0, 0, n, m, k, d, addr, *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                     *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _reference(fleet, lo, hi, k=None, **kw):
    n, m = fleet[0][0].shape
    a, b, rl, rh = gathered(fleet, lo, hi)
    return [x.reshape(n, m * (m - 1) // 2, -1) if x is not None else None for x in sg._sep(a, b, rl, rh, None, k=k, **kw)]


def _scenes(fleet, rows):
    return [[np.ascontiguousarray(x[rows]) for x in axis] for axis in fleet]


# ---------------------------------------------------------------- 1. forward
def test_forward_is_the_pair_entry_bit_for_bit(shape):
    m, n, ks, ds = SHAPES[shape]
    inside = []
    for d in ds:
        fleet = fleet_inputs(n, m, d)
        for k in ks:
            lo, hi = scene_windows(fleet, k, 900 + k)
            want = _reference(fleet, lo, hi)
            got = _fleet(fleet, lo, hi)
            assert sg._all_same(got, want), (shape, d, k)
            # a condition on the inputs, on the reference entry's outputs alone: times strictly inside the clamped window
            first, second = pairs_of(m)
            total = np.min([axis[6] + axis[7] for axis in fleet], axis=0)      # (n, m): a vehicle's shortest axis
            end = np.minimum(total[:, first], total[:, second])[:, :, None]
            finite = np.isfinite(want[0])
            t = want[1]
            within = finite & (t > np.maximum(lo[:, None, :], 0.0)) & (t < np.minimum(hi[:, None, :], end))
            inside.append(within.sum() / max(finite.sum(), 1))
            print("%s d = %d k = %d: %d queries the same bits in value and time; %.0f %% finite, %.0f %% of those strictly inside the window"
                  % (shape, d, k, t.size, 100 * finite.mean(), 100 * inside[-1]))
            if shape != "5x30" or k != 7:
                continue
            # a NULL window end is the infinite one, bit for bit; each output alone, nothing else written (the sentinels behind it)
            inf = np.full(lo.shape, np.inf)
            assert sg._all_same(_fleet(fleet, None, hi), _fleet(fleet, -inf, hi)) and sg._all_same(_fleet(fleet, lo, None), _fleet(fleet, lo, inf))
            assert sg._all_same(_fleet(fleet, None, None, k=k), _fleet(fleet, -inf, inf))
            assert sg._all_same(_fleet(fleet, None, None, k=k), _reference(fleet, None, None, k=k))
            for f in range(2):
                some = _fleet(fleet, lo, hi, want=[g == f for g in range(2)])
                assert some[1 - f] is None and _same_bits(some[f], got[f]), (d, f)
            # NULL end velocities are zeros
            still = [[x.copy() for x in axis] for axis in fleet]
            for axis in still:
                axis[3][:], axis[4][:] = 0.0, 0.0
            assert sg._all_same(_fleet(still, lo, hi, zero_vel=True), _fleet(still, lo, hi))
            assert sg._all_same(_fleet(still, lo, hi, zero_vel=True), _reference(still, lo, hi))
            # the NaN rule: a duration of 0, -1, inf, NaN in one axis of one vehicle makes exactly that vehicle's m - 1 pairs of that scene
            # NaN and changes no other bit
            bad = [[x.copy() for x in axis] for axis in fleet]
            hit = ((3, 0, 0, 6, 0.0), (9, 4, d - 1, 7, -1.0), (17, 2, 0, 7, np.inf), (29, 1, d - 1, 6, np.nan))      # scene, vehicle, axis, field
            poisoned = np.zeros(got[0].shape, dtype=bool)
            for s, v, c, f, value in hit:
                bad[c][f][s, v] = value
                poisoned[s, (first == v) | (second == v), :] = True
            assert poisoned.sum() == len(hit) * (m - 1) * k
            for x, ref in zip(_fleet(bad, lo, hi), got):
                assert np.array_equal(np.isnan(x), poisoned | np.isnan(ref)), d
                assert np.array_equal(_bits(x[~poisoned]), _bits(ref[~poisoned])), d
    print("%s: strictly inside the window: %s" % (shape, ", ".join("%.2f" % x for x in inside)))
    assert min(inside) >= 0.25, inside


# ---------------------------------------------------------------- 2. reproducibility
def test_bits_depend_on_the_scene_and_its_query_only():
    m, n, k = 5, 30, 7
    for d in (1, 2, 3):
        fleet = fleet_inputs(n, m, d)
        lo, hi = scene_windows(fleet, k, 950 + d)
        first = _fleet(fleet, lo, hi)
        assert sg._all_same(first, _fleet(fleet, lo, hi)), "differs from run to run"
        order = np.random.default_rng(5).permutation(n)
        assert sg._all_same(_fleet(_scenes(fleet, order), lo[order], hi[order]), [x[order] for x in first]), d
        for rows in (slice(0, 1), slice(12, 13), slice(29, 30), slice(n - 13, n)):      # single scenes, and the last 13 as a batch of their own
            assert sg._all_same(_fleet(_scenes(fleet, rows), lo[rows], hi[rows]), [x[rows] for x in first]), (d, rows)
        for at in (0, 3, 7):      # the seven columns inside a launch of eight: every query lands in another thread, next to another query
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=1))      # noqa: E731
            eight = _fleet(fleet, wide(lo, 0.1), wide(hi, 0.2))
            assert sg._all_same([np.delete(x, at, axis=2) for x in eight], first), (d, at)
    print("the same bits in any order of the scenes, in any batch and in any launch shape")


# ---------------------------------------------------------------- 3. autograd
def _fleet_leaves(fleet):
    """the eight leaves, (n, m, d) each, in the table's order"""
    return [_t(np.stack([axis[f] for axis in fleet], axis=2)).requires_grad_() for f in range(8)]


def _run(leaves, lo, hi):
    return rp.trajectory_fleet_separation([leaves[f] for f in SIX], lo, hi)


def _pairwise(splines, lo, hi, m):
    """trajectory_separation on the pairs gathered in torch from eight (n, m, d) tensors: (the expanded leaves A (8), B (8), lo, hi -- detached,
    so that each pair's terms stay apart -- and the outputs, (n pairs, k))"""
    n, _, d = splines[0].shape
    first, second = (torch.as_tensor(x, device=splines[0].device) for x in pairs_of(m))
    wide = lambda t, which: t.detach()[:, which, :].reshape(-1, d).clone().requires_grad_()      # noqa: E731
    a, b = [wide(t, first) for t in splines], [wide(t, second) for t in splines]
    rep = lambda w: w.detach().unsqueeze(1).expand(n, len(first), w.shape[1]).reshape(-1, w.shape[1]).clone().requires_grad_()      # noqa: E731
    lo_e, hi_e = rep(lo), rep(hi)
    return a, b, lo_e, hi_e, rp.trajectory_separation([a[f] for f in SIX], [b[f] for f in SIX], lo_e, hi_e, None)


def _folded(per_pair_a, per_pair_b, n, m):
    """a pair's two gradients, (n pairs, d) each, added into its two vehicles, (n, m, d), in longdouble"""
    first, second = pairs_of(m)
    d = per_pair_a.shape[1]
    out = np.zeros((n, m, d), dtype=LD)
    np.add.at(out, (slice(None), first), per_pair_a.reshape(n, len(first), d))
    np.add.at(out, (slice(None), second), per_pair_b.reshape(n, len(first), d))
    return out


def _reference_gradients(splines, lo, hi, m, g):
    """(the gradients of sum(g * sep_sq) in the eight (n, m, d) tensors, lo and hi; the sum of the absolute values of their terms): the pair
    entry's own autograd on the gathered pairs, one backward per query column so that every (pair, query) term stays apart, the terms
    added in longdouble.  Also the pair entry's outputs."""
    n, _, d = splines[0].shape
    k = lo.shape[1]
    a, b, lo_e, hi_e, outs = _pairwise(splines, lo, hi, m)
    leaves = a + b + [lo_e, hi_e]
    total = [np.zeros((n, m, d), dtype=LD) for _ in range(8)] + [np.zeros((n, k), dtype=LD) for _ in range(2)]
    size = [np.zeros_like(x) for x in total]
    pairs = m * (m - 1) // 2
    for q in range(k):
        column = torch.zeros_like(outs[0])
        column[:, q] = g.reshape(-1, k)[:, q]
        terms = [x.cpu().numpy().astype(LD) for x in torch.autograd.grad(outs[0], leaves, grad_outputs=column, retain_graph=True)]
        for f in range(8):
            total[f] += _folded(terms[f], terms[8 + f], n, m)
            size[f] += _folded(np.abs(terms[f]), np.abs(terms[8 + f]), n, m)
        for w in range(2):
            total[8 + w] += terms[16 + w].reshape(n, pairs, k).sum(axis=1)
            size[8 + w] += np.abs(terms[16 + w]).reshape(n, pairs, k).sum(axis=1)
    return total, size, outs


def _assert_close(got, total, size, what):
    """Each gradient within 1e-12 of the sum of |terms|.  lo and hi: the element's own terms -- a (pair, query)'s share of lo_bar is the same
    bits in both computations (the evaluator's tau_bar is pointwise and the axes are added in one order), so only the order of the sum
    over the pairs differs.  The eight gradients of one vehicle and axis come out of one chain rule in the evaluator's reverse kernel,
    applied to sums over that spline's queries that all eight share (reduce_rows), so one of them is exact only to the rounding of
    the largest: its unit is the largest of the eight sums of |terms| of its vehicle and axis.  (Measured: the element's own sum is missed
    by 5.6e-17 absolute on a vel2 whose terms sum to < 6e-5 next to gradients of order 10.)"""
    shared = np.max(np.stack(size[:8]), axis=0)
    worst = 0.0
    for f, (x, ref, s) in enumerate(zip(got, total, size)):
        s = shared if f < 8 else s
        err = np.abs(x.astype(LD) - ref)
        ratio = float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1), 0)))
        print("  %s, input %d: at most %.2e of the sum of |terms|" % (what, f, ratio))
        worst = max(worst, ratio)
        assert np.all(err <= 1e-12 * s), (what, f, float(np.max(err - 1e-12 * s)))
    return worst


def _hand_made_scene():
    """One scene of three vehicles in dyadic numbers after section 24's hand-made cases, for the classes END of the first vehicle and END of
    the second: on axis 0 all run at the constant velocity 2 from 3, 0 and -1; on axis 1 vehicle 0 rises from rest, 0 -> 64 -> 128 in 2 + 2,
    vehicle 1 stands at 1000 and ends at 3, vehicle 2 stands at -1000 and ends at 1.5.  Pair (0, 1): the distance shrinks until the window
    ends with vehicle 1, the second; pair (1, 2): constant, the earliest wins, the start; pair (0, 2): it grows, the start.  With vehicle 0
    cut to 1 + 1 and vehicle 1 left at 3, pair (0, 1) ends with vehicle 0, the first."""
    line = lambda p0, v, d0, d1: (p0, p0 + v * d0, p0 + v * (d0 + d1), v, v, v, d0, d1)      # noqa: E731
    rest = lambda p0, p1, p2, d0, d1, v1: (p0, p1, p2, 0.0, 0.0, v1, d0, d1)      # noqa: E731
    scenes = [
        ([line(3.0, 2.0, 2.0, 2.0), line(0.0, 2.0, 1.0, 2.0), line(-1.0, 2.0, 0.5, 1.0)],
         [rest(0.0, 64.0, 128.0, 2.0, 2.0, 48.0), line(1000.0, 0.0, 2.0, 1.0), line(-1000.0, 0.0, 1.0, 0.5)]),
        ([line(3.0, 2.0, 1.0, 1.0), line(0.0, 2.0, 1.0, 2.0), line(-1.0, 2.0, 2.0, 2.0)],
         [rest(0.0, 16.0, 32.0, 1.0, 1.0, 24.0), line(1000.0, 0.0, 2.0, 1.0), line(-1000.0, 0.0, 2.0, 2.0)]),
    ]
    return [[np.array([[scene[c][v][f] for v in range(3)] for scene in scenes], dtype=np.float64) for f in range(8)] for c in range(2)]


def test_autograd_against_the_pair_entry(d):
    d = int(d)
    m, n, k = 5, 30, 7
    fleet = fleet_inputs(n, m, d)
    lo_np, hi_np = scene_windows(fleet, k, 960 + d)
    leaves = _fleet_leaves(fleet)
    lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
    rng = np.random.default_rng(961)
    g = _t(rng.standard_normal((n, m * (m - 1) // 2, k)))
    outs = _run(leaves, lo, hi)
    assert len(outs) == 2 and outs[0].requires_grad and not outs[1].requires_grad
    every = leaves + [lo, hi]
    total, size, ref_outs = _reference_gradients(leaves, lo, hi, m, g)
    assert _same_bits(outs[0].detach().cpu().numpy().reshape(-1, k), ref_outs[0].detach().cpu().numpy())
    assert _same_bits(outs[1].cpu().numpy().reshape(-1, k), ref_outs[1].cpu().numpy())
    # the classes of the returned times, on the pair entry's times
    a, b, rl, rh = gathered(fleet, lo_np, hi_np)
    ref_t = ref_outs[1].cpu().numpy()
    cls = sr.classes(a, b, rl, rh, np.zeros(rl.shape), ref_t)[0]
    share = np.bincount(cls.ravel(), minlength=7) / cls.size
    print("d = %d: classes of the returned times: LO %.3f HI %.3f END of the first %.3f END of the second %.3f START %.3f interior %.3f none %.3f"
          % ((d,) + tuple(share)))
    for c in (sr.LO, sr.HI, sr.END_A, sr.END_B, sr.OTHER, sr.NONE):
        assert share[c] > 0, c
    got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    again = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], every, grad_outputs=g, retain_graph=True)]
    assert all(_same_bits(x, y) for x, y in zip(got, again)), "backward twice differs"
    assert all(np.isfinite(x).all() for x in got)
    worst = _assert_close(got, total, size, "reverse mode")
    print("d = %d: reverse mode against the pair entry's autograd on the gathered pairs: at most %.2e of the sum of |terms|, asserted 1e-12" % (d, worst))
    # a NaN value has gradient exactly 0
    miss = torch.isnan(outs[0].detach())
    assert int(miss.sum()) > 0
    for x in torch.autograd.grad(outs[0], every, grad_outputs=torch.where(miss, g, torch.zeros_like(g)), retain_graph=True):
        assert float(x.abs().max()) == 0.0
    # forward mode, torch.func.jvp, duality
    dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal((n, k))) for _ in range(2)]
    with fwAD.dual_level():
        dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
        douts = _run(dual[:8], dual[8], dual[9])
        got_dot = fwAD.unpack_dual(douts[0]).tangent.cpu().numpy()
        assert fwAD.unpack_dual(douts[1]).tangent is None
    _, func_dot = torch.func.jvp(lambda *xs: _run(list(xs[:8]), xs[8], xs[9])[0], tuple(x.detach() for x in every), tuple(dots))
    assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss.cpu().numpy())
    # against the pair entry's forward mode on the gathered pairs: per query one term per input, the same terms
    first, second = (torch.as_tensor(x, device=g.device) for x in pairs_of(m))
    gather = lambda t, which: t[:, which, :].reshape(-1, d)      # noqa: E731
    rep = lambda w: w.unsqueeze(1).expand(n, len(first), k).reshape(-1, k)      # noqa: E731
    with fwAD.dual_level():
        dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
        pa, pb = [gather(t, first) for t in dual[:8]], [gather(t, second) for t in dual[:8]]
        ref_dot = fwAD.unpack_dual(rp.trajectory_separation([pa[f] for f in SIX], [pb[f] for f in SIX], rep(dual[8]), rep(dual[9]), None)[0]).tangent
        ref_dot = ref_dot.cpu().numpy().reshape(got_dot.shape)
    gn, dn = g.cpu().numpy(), [t.cpu().numpy() for t in dots]
    left_terms = [np.where(np.isnan(got_dot), 0, gn.astype(LD) * got_dot)]
    right_terms = [x.astype(LD) * t for x, t in zip(got, dn)]
    left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
    scale = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
    ref_left = float(np.where(np.isnan(ref_dot), 0, gn.astype(LD) * ref_dot).sum())
    print("d = %d: duality between reverse and forward mode: %.2e of the sum of |terms|; forward mode against the pair entry's: %.2e"
          % (d, abs(left - right) / scale, abs(left - ref_left) / scale))
    assert abs(left - right) <= 1e-12 * scale and abs(left - ref_left) <= 1e-12 * scale
    assert np.array_equal(np.isnan(ref_dot), np.isnan(got_dot))
    # first order only
    (g0,) = torch.autograd.grad((torch.nan_to_num(_run(leaves, lo, hi)[0]) ** 2).sum(), leaves[1], create_graph=True)
    try:
        g0.sum().backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("double backward did not raise")
    if d != 2:
        torch.cuda.synchronize()
        return
    # the hand-made scenes: the END of the pair's second vehicle and of its first, whatever the family holds; a (k,) window, six tensors
    hand = _hand_made_scene()
    hl = _fleet_leaves(hand)
    outs = _run(hl, None, None)
    a, b, _, _ = gathered(hand, None, None)
    whole = np.full((6, 1), np.inf)
    cls, axis = sr.classes(a, b, -whole, whole, np.zeros((6, 1)), outs[1].cpu().numpy().reshape(6, 1))
    print("hand-made scenes: times %s, classes %s" % (outs[1].cpu().numpy().ravel(), cls.ravel()))
    assert cls[0, 0] == sr.END_B and cls[3, 0] == sr.END_A and outs[1][0, 0, 0].item() == 3.0 and outs[1][1, 0, 0].item() == 2.0
    total, size, ref_outs = _reference_gradients(hl, _t(-np.full((2, 1), np.inf)), _t(np.full((2, 1), np.inf)), 3, torch.ones_like(outs[0]))
    got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0].sum(), hl)]
    _assert_close(got, total[:8], size[:8], "hand-made scenes")
    assert got[6][0, 1, 0] != 0 and got[7][0, 1, 0] != 0 and got[6][1, 0, 0] != 0 and got[7][1, 0, 0] != 0      # the ends' durations take the time's share
    row = _t(np.array([0.25, 0.5])).requires_grad_()
    six = [hl[f].detach() for f in SIX[:6]]
    o = rp.trajectory_fleet_separation(six, row, None)
    assert o[0].shape == (2, 3, 2)
    (g_row,) = torch.autograd.grad(o[0].sum(), row)
    assert g_row.shape == (2,) and torch.isfinite(g_row).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. through the solves
def test_the_pipeline_is_the_composition():
    """min_time_fleet_separation (m = 3, d = 2, n = 100, synchronised) on golden problems: the bits of min_time_solve + synchronize_axes +
    trajectory_fleet_separation composed by hand; its gradient in pos1 finite, and within 1e-12 of the sum of |terms| of the same
    composition with the pair entry on the gathered pairs, a term being one (pair, query)'s share of the gradient and the unit the
    largest such sum among the vehicle's axes (_assert_close's reason, and the stretch to the slowest axis couples them)."""
    n, m, d, k = 100, 3, 2, 8
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
    out = rp.min_time_fleet_separation(x, lo, hi, gap_tol=1e-13)
    assert len(out) == 3 and len(out[2]) == 5 and all(t.shape == (n, m, d) for t in out[2])
    six, sol = spline_of(x)
    by_hand = rp.trajectory_fleet_separation(six, lo, hi)
    assert _same_bits(out[0].detach().cpu().numpy(), by_hand[0].detach().cpu().numpy()) and _same_bits(out[1].cpu().numpy(), by_hand[1].cpu().numpy())
    assert all(_same_bits(p.detach().cpu().numpy().astype(np.float64), q.detach().cpu().numpy().reshape(n, m, d).astype(np.float64)) for p, q in zip(out[2], sol))
    finite = torch.isfinite(out[0].detach())
    print("%d of %d scenes solved finite, %.0f %% of the queries finite" % (int(good.sum()), n, 100 * float(finite.float().mean())))
    assert good.mean() > 0.95 and float(finite.float().mean()) > 0.9
    g = _t(np.random.default_rng(971).uniform(0.5, 1.5, tuple(out[0].shape)))
    g = torch.where(finite, g, torch.zeros_like(g))
    (got,) = torch.autograd.grad(out[0], x[1], grad_outputs=g)
    ok = _t(good).bool()[:, None, None].expand_as(got)
    assert torch.isfinite(got[ok]).all()
    # the reference: the same composition, the pair entry on the gathered pairs; one backward per (pair, query) through the solve
    eight = six[:3] + [torch.zeros_like(six[0]), torch.zeros_like(six[0])] + six[3:]
    a, b, lo_e, hi_e, outs = _pairwise(eight, lo, hi, m)
    pairs = m * (m - 1) // 2
    first, second = pairs_of(m)
    total, size = np.zeros((n, m, d), dtype=LD), np.zeros((n, m, d), dtype=LD)
    table = (0, 1, 2, 5, 6, 7)      # the six of synchronize_axes in the table's order
    g_flat = g.reshape(n * pairs, k)
    for q in range(k):
        column = torch.zeros_like(outs[0])
        column[:, q] = g_flat[:, q]
        terms = torch.autograd.grad(outs[0], [a[f] for f in table] + [b[f] for f in table], grad_outputs=column, retain_graph=True)
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
    print("d sep_sq / d pos1 through the pipeline against the same composition with the pair entry: at most %.2e of the sum of |terms|, asserted 1e-12" % worst)
    assert np.all(err[rows] <= 1e-12 * size[rows])
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
