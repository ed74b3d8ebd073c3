"""The cases of tests/test_gpu_fleet_cull.py, each run in a fresh process (`python tests/fleet_cull_gpu_cases.py <case> [arguments]`), on
top of tests/fleet_gpu_cases.py's inputs and tests/fleet_contact_gpu_cases.py's un-culled entry.  Not collected by pytest (no test_ prefix
on the file).  What is checked, and why each bound is what it is: DESIGN.md section 30.  The reference throughout is the un-culled entry,
rp_trajectory_fleet_contact / trajectory_fleet_contact(broad_phase=False), on the same inputs: every bit of every time and rate, NaN bits
included.  The conditions on the inputs -- how many pairs have a contact, how many are provably far -- come from that entry's output and
from the longdouble boxes of extrema_ref.extrema_ld alone.

The spread family: fleet_gpu_cases.fleet_inputs(n, m, d) with vehicle v moved by spacing times its grid cell -- side = ceil(m ** (1 / d)),
coordinate (v // side ** c) % side on axis c, added to pos0, pos1, pos2 -- windows scene_windows(fleet, k, 900 + k), the per-scene level
3.0 ** 2 everywhere, the per-pair level (r_i + r_j) ** 2 with r_v = 1.25 + 0.5 (v mod 2)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_contact_gpu_cases as fc  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import extrema_ref as er  # noqa: E402
import fleet_gpu_cases as fg  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

LD = np.longdouble
SIX, SHAPES, LAYOUTS = fg.SIX, fg.SHAPES, fc.LAYOUTS
_t, _bits, _same_bits, Out, _all_same = fg._t, fg._bits, fg._same_bits, fg.Out, fg.sg._all_same
fleet_inputs, scene_windows, pairs_of = fg.fleet_inputs, fg.scene_windows, fg.pairs_of
SPACING, ROOM = 6.0, 1e-6
GUARD = 16      # words behind the flags and the list, and what they hold
FLAG_GUARD, LIST_GUARD = 0xA5, 0xDEADBEEF


def spread(fleet, spacing=SPACING):
    """The fleet with vehicle v moved to its grid cell."""
    n, m = fleet[0][0].shape
    d = len(fleet)
    side = int(np.ceil(m ** (1.0 / d) - 1e-9))
    while side ** d < m:
        side += 1
    out = [[x.copy() for x in axis] for axis in fleet]
    v = np.arange(m)
    for c in range(d):
        cell = (v // side ** c) % side
        for f in (0, 1, 2):
            out[c][f] += spacing * cell[None, :]
    return out


def spread_inputs(n, m, d, k, spacing=SPACING):
    """(fleet, lo, hi, {layout: level}) of the spread family."""
    fleet = spread(fleet_inputs(n, m, d), spacing)
    lo, hi = scene_windows(fleet, k, 900 + k)
    first, second = pairs_of(m)
    r = 1.25 + 0.5 * (np.arange(m) % 2)
    per_pair = np.ascontiguousarray(np.broadcast_to(((r[first] + r[second]) ** 2)[None, :, None], (n, len(first), k)))
    return fleet, lo, hi, {"per pair": per_pair, "per scene": np.full((n, k), 3.0 ** 2)}


def _culled(fleet, level, lo, hi, want_rate=True, zero_vel=False):
    """The culled entry: (time, rate or None, kept (n, pairs) bool, the list's first `count` entries, count).  The outputs are pre-filled
    with Out's sentinel and the words behind them, the flags and the list are looked at afterwards."""
    n, m = fleet[0][0].shape
    d, k = len(fleet), level.shape[-1]
    pairs = m * (m - 1) // 2
    tf = [[_t(x) for x in axis] for axis in fleet]
    tv, tl, th = (_t(x) if x is not None else None for x in (level, lo, hi))
    outs = [Out(n, pairs, k), Out(n, pairs, k) if want_rate else None]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    size = capi.trajectory_fleet_contact_culled_workspace(n, m, k, d)
    work = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device=fg.sg.tg.DEV)      # whatever it held before does not matter
    kept = torch.full((n * pairs + GUARD,), FLAG_GUARD, dtype=torch.uint8, device=work.device)
    listed = torch.full((n * pairs + GUARD,), LIST_GUARD - (1 << 32), dtype=torch.int32, device=work.device)      # uint32 words
    count = torch.full((1 + GUARD,), LIST_GUARD - (1 << 32), dtype=torch.int32, device=work.device)
    torch.cuda.synchronize()
    capi.trajectory_fleet_contact_culled(0, 0, n, m, k, d, addr, tv.data_ptr(), int(level.ndim == 3),
                                         *[t.data_ptr() if t is not None else 0 for t in (tl, th)], *[o.ptr if o else 0 for o in outs],
                                         work.data_ptr(), size, kept.data_ptr(), listed.data_ptr(), count.data_ptr())
    torch.cuda.synchronize()
    assert bool((work[size:] == 0x5A).all()), "the bytes behind the workspace were written"
    kept = kept.cpu().numpy()
    listed, count = (x.cpu().numpy().view(np.uint32).astype(np.int64) for x in (listed, count))
    assert np.all(kept[n * pairs:] == FLAG_GUARD) and np.all(listed[n * pairs:] == LIST_GUARD) and np.all(count[1:] == LIST_GUARD)
    assert set(np.unique(kept[:n * pairs])) <= {0, 1}
    assert 0 <= count[0] <= n * pairs
    return [o.get() if o else None for o in outs] + [kept[:n * pairs].reshape(n, pairs) != 0, listed[:count[0]].copy(), int(count[0])]


def _check_list(kept, listed, count, what):
    """The list is strictly increasing, is the kept flags' indices, and the count is its length."""
    assert count == len(listed) == int(kept.sum()), what
    assert np.array_equal(listed, np.flatnonzero(kept.reshape(-1))), what
    assert np.all(np.diff(listed) > 0), what


def _same_as_unculled(fleet, level, lo, hi, what, **kw):
    """The culled entry against the un-culled one on the same inputs: (the un-culled outputs, kept, the list, the count)."""
    want = fc._enc(fleet, level, lo, hi, **kw)
    time, rate, kept, listed, count = _culled(fleet, level, lo, hi, **kw)
    assert _same_bits(time, want[0]), what
    assert (rate is None and want[1] is None) or _same_bits(rate, want[1]), what
    assert not np.any(time == fg.sg.tg.SENTINEL) and (rate is None or not np.any(rate == fg.sg.tg.SENTINEL)), what
    _check_list(kept, listed, count, what)
    # no culled pair has a finite time, and every pair with one is in the list
    assert not np.isfinite(want[0][~kept]).any(), what
    return want, kept, listed, count


def boxes_ld(fleet, lo, hi):
    """extrema_ref.extrema_ld's pos_min and pos_max per axis, (n, m, k) longdouble each, the scene's windows repeated per vehicle."""
    n, m = fleet[0][0].shape
    rep = lambda w: np.repeat(w, m, axis=0) if w is not None else None      # noqa: E731
    out = []
    for axis in fleet:
        values, _ = er.extrema_ld([x.reshape(-1) for x in axis], rep(lo), rep(hi))
        out.append((np.asarray(values[0], dtype=LD).reshape(n, m, -1), np.asarray(values[1], dtype=LD).reshape(n, m, -1)))
    return out


def far_ld(fleet, level, lo, hi, room=ROOM):
    """(n, pairs) bool: the pairs whose longdouble boxes are further apart than level (1 + room) in all k queries."""
    m = fleet[0][0].shape[1]
    first, second = pairs_of(m)
    total = None
    with np.errstate(all="ignore"):
        for low, high in boxes_ld(fleet, lo, hi):
            gap = np.maximum(np.maximum(low[:, first] - high[:, second], low[:, second] - high[:, first]), LD(0))
            gap = np.where(np.isnan(low[:, first] + high[:, second] + low[:, second] + high[:, first]), LD(np.nan), gap)
            total = gap * gap if total is None else total + gap * gap
        wide = np.asarray(level, dtype=LD) if level.ndim == 3 else np.asarray(level, dtype=LD)[:, None, :]
        return np.all(total > wide * (1 + LD(room)), axis=2)


def _shares(want, far, what, finite_least, far_least):
    """The conditions on the inputs: the share of pairs with at least one finite time (the un-culled entry's) and of box-far pairs."""
    finite = float(np.isfinite(want[0]).any(axis=2).mean())
    share = float(far.mean())
    print("  %s: %.1f %% of the pairs have a finite time, %.1f %% are box-far in longdouble" % (what, 100 * finite, 100 * share))
    assert finite >= finite_least and share >= far_least, (what, finite, share)
    assert not np.isfinite(want[0][far]).any(), what      # no far pair has a finite time
    return finite, share


# ---------------------------------------------------------------- 1. forward
def test_forward_is_the_unculled_entry_bit_for_bit(shape, d):
    m, n, ks, _ = SHAPES[shape]
    d = int(d)
    first, second = pairs_of(m)
    small = shape != "64x1"
    for k in ks:
        fleet, lo, hi, both = spread_inputs(n, m, d, k)
        for layout, level in both.items():
            what = (shape, d, k, layout)
            want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, what)
            far = far_ld(fleet, level, lo, hi)
            _shares(want, far, "%s d = %d k = %d, level %s" % what, 0.07 if small else 0.02, 0.07 if small else 0.80)
            assert not kept[far].any(), what      # every pair that is box-far with 1e-6 room is culled
            print("%s d = %d k = %d, level %s: %d queries the same bits in time and rate; %d of %d pairs went to the search"
                  % (shape, d, k, layout, want[0].size, count, kept.size))
            if shape != "5x30" or k != 7:
                continue
            # NULL window ends, no rate, NULL end velocities: each the un-culled entry's bits on the same call
            _same_as_unculled(fleet, level, None, hi, what)
            _same_as_unculled(fleet, level, lo, None, what)
            _same_as_unculled(fleet, level, None, None, what)
            alone, _, _, _ = _same_as_unculled(fleet, level, lo, hi, what, want_rate=False)
            assert alone[1] is None and _same_bits(alone[0], want[0])
            still = [[x.copy() for x in axis] for axis in fleet]
            for axis in still:
                axis[3][:], axis[4][:] = 0.0, 0.0
            assert _all_same(_same_as_unculled(still, level, lo, hi, what, zero_vel=True)[0], fc._enc(still, level, lo, hi))
            # the NaN rule: fleet_contact_gpu_cases' hits -- a duration of 0, -1, inf, NaN in one axis of one vehicle
            bad = [[x.copy() for x in axis] for axis in fleet]
            hit = ((3, 0, 0, 6, 0.0), (9, 4, d - 1, 7, -1.0), (17, 2, 0, 7, np.inf), (29, 1, d - 1, 6, np.nan))      # scene, vehicle, axis, field
            poisoned = np.zeros(want[0].shape, dtype=bool)
            for s, v, c, f, value in hit:
                bad[c][f][s, v] = value
                poisoned[s, (first == v) | (second == v), :] = True
            got_bad, kept_bad, _, _ = _same_as_unculled(bad, level, lo, hi, what)
            assert np.array_equal(np.isnan(got_bad[0]), poisoned | np.isnan(want[0])), what
            assert kept_bad[poisoned.all(axis=2)].all(), what      # a NaN box keeps the pair: the search makes the NaN
            if layout != "per scene":
                continue
            # spoilt levels: NaN, +inf, -1, -inf
            spoilt = level.copy()
            for s, q, value in ((2, 0, np.nan), (11, 3, np.inf), (20, 6, -1.0), (29, 6, -np.inf)):
                spoilt[s, q] = value
            _, kept_spoilt, _, _ = _same_as_unculled(fleet, spoilt, lo, hi, what)
            assert kept_spoilt[[2, 11, 29]].all(), what      # a NaN or infinite level is not far


# ---------------------------------------------------------------- 2. the sieve's answer
def _reach(fleet, lo, hi, k):
    """rp_trajectory_fleet_reach: (box_min, box_max), d arrays of (n, m, k) each."""
    n, m = fleet[0][0].shape
    d = len(fleet)
    tf = [[_t(x) for x in axis] for axis in fleet]
    tl, th = (_t(x) if x is not None else None for x in (lo, hi))
    outs = [[Out(n, m, k) for _ in range(d)] for _ in range(2)]
    capi.trajectory_fleet_reach(0, 0, n, m, k, d, [t.data_ptr() for axis in tf for t in axis], *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                [o.ptr for o in outs[0]], [o.ptr for o in outs[1]])
    torch.cuda.synchronize()
    return [[o.get() for o in side] for side in outs]


def _extrema(fleet, lo, hi, k):
    """rp_trajectory_extrema's pos_min and pos_max on the n m splines of each axis with the windows repeated per vehicle."""
    n, m = fleet[0][0].shape
    rep = lambda w: _t(np.repeat(w, m, axis=0)) if w is not None else None      # noqa: E731
    tl, th = rep(lo), rep(hi)
    out = [[], []]
    for axis in fleet:
        ts = [_t(x.reshape(-1)) for x in axis]
        low, high = Out(n, m, k), Out(n, m, k)
        capi.trajectory_extrema(0, 0, n * m, k, [t.data_ptr() for t in ts], *[t.data_ptr() if t is not None else 0 for t in (tl, th)],
                                [low.ptr, high.ptr, 0, 0], None)
        torch.cuda.synchronize()
        out[0].append(low.get())
        out[1].append(high.get())
    return out


def test_the_sieves_answer(shape, d):
    m, n, ks, _ = SHAPES[shape]
    d, k = int(d), (1 if shape == "64x1" else 7)
    fleet, lo, hi, both = spread_inputs(n, m, d, k)
    # the boxes: rp_trajectory_extrema's bits on the n m splines, with both windows, one and none
    for wl, wh in ((lo, hi), (None, hi), (lo, None), (None, None)):
        kk = k if (wl is not None or wh is not None) else 1
        assert all(_all_same(x, y) for x, y in zip(_reach(fleet, wl, wh, kk), _extrema(fleet, wl, wh, kk))), (shape, d)
    six = [_t(np.stack([axis[f] for axis in fleet], axis=2)) for f in range(8)]
    box_min, box_max = rp.trajectory_fleet_reach([six[f] for f in SIX], _t(lo), _t(hi))
    want_min, want_max = _reach(fleet, lo, hi, k)
    assert box_min.shape == box_max.shape == (n, m, k, d) and not box_min.requires_grad
    assert _same_bits(box_min.cpu().numpy(), np.stack(want_min, axis=3)) and _same_bits(box_max.cpu().numpy(), np.stack(want_max, axis=3))
    for layout, level in both.items():
        what = (shape, d, layout)
        want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, what)
        far = far_ld(fleet, level, lo, hi)
        assert not kept[far].any(), what
        assert far.mean() >= (0.80 if shape == "64x1" else 0.07), what
        again = _culled(fleet, level, lo, hi)      # the same list and bits in two runs
        assert _all_same(again[:2], want) and np.array_equal(again[2], kept) and np.array_equal(again[3], listed) and again[4] == count
        flags = rp.fleet_contact_candidates([six[f] for f in SIX], None, _t(lo), _t(hi), level_sq=_t(level))
        assert flags.dtype == torch.bool and flags.shape == kept.shape and np.array_equal(flags.cpu().numpy(), kept), what
        by_radius = rp.fleet_contact_candidates([six[f] for f in SIX[:6]], _t(np.sqrt(level)), _t(lo), _t(hi))
        assert by_radius.shape == kept.shape
        print("%s d = %d, level %s: %d of %d pairs kept, %.1f %% box-far in longdouble, all of those culled; the flags, the list and the count "
              "agree and repeat" % (shape, d, layout, count, kept.size, 100 * far.mean()))


# ---------------------------------------------------------------- 3. the ends of the range
def test_nothing_to_cull():
    """spacing = 0: section 27's own family.  Whatever is kept, the bits are the un-culled ones; at least 90 % of the pairs are not box-far
    in longdouble (with no room either way), so at least that many are kept."""
    m, n, d, k = 5, 30, 2, 7
    fleet, lo, hi, both = spread_inputs(n, m, d, k, spacing=0.0)
    for layout, level in both.items():
        want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, layout)
        near = ~far_ld(fleet, level, lo, hi, room=-1e-6)      # not even far with 1e-6 taken off the level
        assert near.mean() >= 0.90 and kept[near].all(), (layout, near.mean())
        print("spacing 0, level %s: %.1f %% of the pairs cannot be far, %d of %d kept" % (layout, 100 * near.mean(), count, kept.size))


def test_everything_culled():
    """spacing = 1000: every pair is culled, the count is 0 and the search has no work: all NaN, the un-culled entry's bits.  With k = 1
    and k = 2 every window of the family is the whole domain.  With k = 7 about one window in a hundred lies before t = 0, where the boxes
    are NaN and the sieve keeps the scene's pairs for the search to make the NaN: exactly those pairs are kept."""
    for m, n, d, k in ((5, 30, 2, 2), (3, 43, 3, 1), (2, 300, 1, 2), (5, 30, 2, 7)):
        fleet, lo, hi, both = spread_inputs(n, m, d, k, spacing=1000.0)
        for layout, level in both.items():
            want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, (m, n, layout))
            assert np.isnan(want[0]).all() and np.isnan(want[1]).all()
            assert np.array_equal(kept, ~far_ld(fleet, level, lo, hi)), (m, n, layout)
            if k <= 2:
                assert count == 0 and not kept.any() and len(listed) == 0, (m, n, layout)
            print("spacing 1000, %d x %d, d = %d, k = %d, level %s: %d of %d pairs kept" % (m, n, d, k, layout, count, kept.size))


def test_the_largest_fleet():
    """m = 256, n = 2, d = 2, k = 1: 65,280 problems, a list that crosses scan chunks and scenes."""
    m, n, d, k = 256, 2, 2, 1
    fleet, lo, hi, both = spread_inputs(n, m, d, k)
    for layout, level in both.items():
        want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, layout)
        far = far_ld(fleet, level, lo, hi)
        assert not kept[far].any()
        assert kept.size == 65280 and count > 2048 // 8 and kept[0].any() and kept[1].any()
        assert len(set(listed // 2048)) > 1      # entries from more than one chunk of flags
        print("m = 256, level %s: %d of %d pairs kept, %.1f %% box-far in longdouble, %.1f %% with a finite time"
              % (layout, count, kept.size, 100 * far.mean(), 100 * np.isfinite(want[0]).any(axis=2).mean()))


# ---------------------------------------------------------------- 4. at the radius
def _radius_scenes():
    """Scenes of three vehicles in two axes in dyadic numbers, r = 4 (level 16).  Scene 0: three standing vehicles (pos0 = pos1 = pos2, no
    velocity), vehicles 1 and 2 at distance exactly r from vehicle 0.  Scenes 1-4: the same with r (1 + 2^-j), j = 10, 30, 45, 52.  Scene 5:
    vehicle 0 runs along axis 0 at the constant velocity 4 from -8 over 1 + 3 and passes vehicle 1, which stands at (0, r), at exactly r
    at t = 2, and vehicle 2, which stands at (0, -r (1 + 2^-40))."""
    stand = lambda p, d0=1.0, d1=1.0: (p, p, p, 0.0, 0.0, 0.0, d0, d1)      # noqa: E731
    line = lambda p0, v, d0, d1: (p0, p0 + v * d0, p0 + v * (d0 + d1), v, v, v, d0, d1)      # noqa: E731
    r = 4.0
    scenes = []
    for j in (None, 10, 30, 45, 52):
        far = r if j is None else r * (1.0 + 2.0 ** -j)
        scenes.append(([stand(0.0), stand(far), stand(0.0)], [stand(0.0), stand(0.0), stand(-far)]))
    scenes.append(([line(-8.0, 4.0, 1.0, 3.0), stand(0.0, 2.0, 2.0), stand(0.0, 2.0, 2.0)],
                   [stand(0.0, 1.0, 3.0), stand(r, 2.0, 2.0), stand(-r * (1.0 + 2.0 ** -40), 2.0, 2.0)]))
    return [[np.array([[scene[c][v][f] for v in range(3)] for scene in scenes], dtype=np.float64) for f in range(8)] for c in range(2)]


def test_at_the_radius():
    fleet = _radius_scenes()
    n = fleet[0][0].shape[0]
    for lo, hi in ((None, None), (np.tile([0.0, 0.5], (n, 1)), np.tile([10.0, 1.5], (n, 1)))):
        k = 1 if lo is None else 2
        for level in (np.full((n, k), 16.0), np.full((n, 3, k), 16.0)):
            want, kept, listed, count = _same_as_unculled(fleet, level, lo, hi, "at the radius")
            start = np.zeros(k) if lo is None else lo[0]
            # standing at exactly r: the window's start, and kept
            assert np.array_equal(want[0][0, 0], start) and np.array_equal(want[0][0, 1], start) and kept[0, 0] and kept[0, 1]
            assert kept[np.isfinite(want[0]).any(axis=2)].all()      # any pair with a finite time is in the list
            print("at the radius, k = %d, level %s: times %s; kept %s" % (k, LAYOUTS[level.ndim == 2], want[0][:, :, 0].tolist(), kept.astype(int).tolist()))


# ---------------------------------------------------------------- 5. torch
def test_torch_broad_phase_is_the_same_bits():
    m, n, d, k = 5, 30, 2, 7
    pairs = m * (m - 1) // 2
    fleet, lo_np, hi_np, both = spread_inputs(n, m, d, k)
    rng = np.random.default_rng(977)
    g = _t(rng.standard_normal((n, pairs, k)))
    lo, hi = _t(lo_np), _t(hi_np)
    for layout, level_np in both.items():
        for by_radius in (False, True):
            leaves = fg._fleet_leaves(fleet)
            query = _t(np.sqrt(level_np) if by_radius else level_np).requires_grad_()
            run = lambda xs, q, on: rp.trajectory_fleet_contact([xs[f] for f in SIX], q if by_radius else None, lo, hi,      # noqa: E731
                                                                level_sq=None if by_radius else q, broad_phase=on)
            off, on = run(leaves, query, False), run(leaves, query, True)
            assert on.shape == (n, pairs, k) and on.requires_grad
            assert _same_bits(on.detach().cpu().numpy(), off.detach().cpu().numpy()), (layout, by_radius)
            finite = float(torch.isfinite(off.detach()).any(dim=2).double().mean())
            assert finite >= 0.07, finite
            every = leaves + [query]
            want = torch.autograd.grad(off, every, grad_outputs=g)
            got = torch.autograd.grad(on, every, grad_outputs=g)
            assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want)), (layout, by_radius)
            assert any(float(x.abs().max()) > 0 for x in got)
            dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal(level_np.shape))]
            tangents = []
            for flag in (False, True):
                with fwAD.dual_level():
                    dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
                    tangents.append(fwAD.unpack_dual(run(dual[:8], dual[8], flag)).tangent.cpu().numpy())
            assert _same_bits(tangents[0], tangents[1]), (layout, by_radius)
            assert np.isfinite(tangents[1]).any()
            print("torch, level %s, %s: broad_phase=True gives the same bits in the times, in 9 gradients and in the tangents; %.1f %% of the "
                  "pairs have a finite time" % (layout, "radius=" if by_radius else "level_sq=", 100 * finite))
    kept = rp.fleet_contact_candidates([fg._fleet_leaves(fleet)[f] for f in SIX], None, lo, hi, level_sq=_t(both["per scene"]))
    assert 0.07 <= 1.0 - float(kept.double().mean())      # the option had something to cull
    # through the solves: section 26's pipeline case on golden problems, the level of fleet_contact_gpu_cases' pipeline case
    n, m, d, k = 100, 3, 2, 8
    pos = gg._golden_positions(n * m * d).reshape(n, m, d, 3)
    x = [_t(pos[..., c]).requires_grad_() for c in range(3)]
    with torch.no_grad():
        sol = rp.min_time_solve(*[t.reshape(-1) for t in x], gap_tol=1e-13)
        six, _ = rp.synchronize_axes([t.reshape(n * m, d) for t in list(x) + [s.reshape(n, m, d) for s in sol[:3]]])
        six = [t.reshape(n, m, d) for t in six]
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
        at = lo.unsqueeze(1).expand(n, m, k).reshape(n * m, k).contiguous()
        start = torch.zeros_like(least)
        for c in range(d):
            p = rp.trajectory_eval(*[t[:, :, c].reshape(n * m) for t in six], at)[0].reshape(n, m, k)
            start = start + (p[:, first, :] - p[:, second, :]) ** 2
    level = _t(fc.scene_levels(((least + start) / 2).cpu().numpy()))
    outs = [rp.min_time_fleet_contact(x, None, lo, hi, level_sq=level, gap_tol=1e-13, broad_phase=flag) for flag in (False, True)]
    assert _same_bits(outs[0][0].detach().cpu().numpy(), outs[1][0].detach().cpu().numpy())
    assert float(torch.isfinite(outs[0][0].detach()).double().mean()) >= 0.25
    grads = [torch.autograd.grad(torch.nan_to_num(o[0]).sum(), x[1], retain_graph=True)[0].cpu().numpy() for o in outs]
    assert _same_bits(grads[0], grads[1])
    print("min_time_fleet_contact(broad_phase=True) on the golden problems: the same bits in the times and in d / d pos1")
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
