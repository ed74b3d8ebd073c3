"""The cases of tests/test_gpu_staggered_cull.py, each run in a fresh process (`python tests/staggered_cull_gpu_cases.py <case> [arguments]`),
on top of tests/staggered_gpu_cases.py's un-culled entry and tests/staggered_cull_inputs.py's inputs.  Not collected by pytest (no test_
prefix on the file).  What is checked, and why each bound is what it is: DESIGN.md section 31.  The reference throughout is the un-culled
entry, rp_trajectory_fleet_contact_staggered / trajectory_fleet_contact(start=, broad_phase=False), on the same inputs: every bit of
every time, local time and rate, NaN bits included.  The conditions on the inputs come from that entry's output and from
staggered_cull_inputs' longdouble statements alone."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import staggered_gpu_cases as sc  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import fleet_contact_gpu_cases as fc  # noqa: E402
import fleet_gpu_cases as fg  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import staggered_cull_inputs as ci  # noqa: E402
import staggered_inputs as si  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

SIX, SHAPES = fg.SIX, ci.SHAPES
_t, _bits, _same_bits, Out, _all_same = fg._t, fg._bits, fg._same_bits, fg.Out, fg.sg._all_same
pairs_of = ci.pairs_of
DEV, SENTINEL = fg.sg.tg.DEV, fg.sg.tg.SENTINEL
GUARD = 16      # words behind the flags and the list, and what they hold
FLAG_GUARD, LIST_GUARD = 0xA5, 0xDEADBEEF
ALL = (True, True, True)


def _culled(fleet, start, level, lo, hi, want=ALL, zero_vel=False):
    """The culled entry: ([time, time_local, rate] with None where not asked for, kept (n, pairs) bool, the list's first `count` entries,
    count).  The outputs are pre-filled with Out's sentinel; the words behind them, the workspace, the flags, the list and the count are
    looked at afterwards."""
    n, m = start.shape
    d, k = len(fleet), level.shape[-1]
    pairs = m * (m - 1) // 2
    tf = [[_t(x) for x in axis] for axis in fleet]
    ts, tv, tl, th = (_t(x) if x is not None else None for x in (start, level, lo, hi))
    outs = [Out(n, pairs, k) if w else None for w in want]
    addr = [0 if zero_vel and f in (3, 4) else t.data_ptr() for axis in tf for f, t in enumerate(axis)]
    size = capi.trajectory_fleet_contact_staggered_culled_workspace(n, m, k, d)
    work = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device=DEV)      # whatever it held before does not matter
    kept = torch.full((n * pairs + GUARD,), FLAG_GUARD, dtype=torch.uint8, device=DEV)
    listed = torch.full((n * pairs + GUARD,), LIST_GUARD - (1 << 32), dtype=torch.int32, device=DEV)      # uint32 words
    count = torch.full((1 + GUARD,), LIST_GUARD - (1 << 32), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    capi.trajectory_fleet_contact_staggered_culled(0, 0, n, m, k, d, addr, ts.data_ptr(), tv.data_ptr(), int(level.ndim == 3),
                                                   *[t.data_ptr() if t is not None else 0 for t in (tl, th)], *[o.ptr if o else 0 for o in outs],
                                                   work.data_ptr(), size, kept.data_ptr(), listed.data_ptr(), count.data_ptr())
    torch.cuda.synchronize()
    assert bool((work[size:] == 0x5A).all()), "the bytes behind the workspace were written"
    kept = kept.cpu().numpy()
    listed, count = (x.cpu().numpy().view(np.uint32).astype(np.int64) for x in (listed, count))
    assert np.all(kept[n * pairs:] == FLAG_GUARD) and np.all(listed[n * pairs:] == LIST_GUARD) and np.all(count[1:] == LIST_GUARD)
    assert set(np.unique(kept[:n * pairs])) <= {0, 1}
    assert 0 <= count[0] <= n * pairs
    return [o.get() if o else None for o in outs], kept[:n * pairs].reshape(n, pairs) != 0, listed[:count[0]].copy(), int(count[0])


def _check_list(kept, listed, count, what):
    """The list is strictly increasing, is the kept flags' indices, and the count is its length."""
    assert count == len(listed) == int(kept.sum()), what
    assert np.array_equal(listed, np.flatnonzero(kept.reshape(-1))), what
    assert np.all(np.diff(listed) > 0), what


def _same_as_unculled(fleet, start, level, lo, hi, what, want=ALL, zero_vel=False, reference=None):
    """The culled entry against the un-culled one on the same inputs: (the un-culled [time, time_local, rate], kept, the list, the count)."""
    ref = reference if reference is not None else sc._rdv(fleet, start, level, lo, hi, zero_vel=zero_vel)
    got, kept, listed, count = _culled(fleet, start, level, lo, hi, want=want, zero_vel=zero_vel)
    for x, y, w in zip(got, ref, want):
        assert (x is None) == (not w), what
        if w:
            assert _same_bits(x, y), what
            assert not np.any(x == SENTINEL), what      # no element left unwritten
    _check_list(kept, listed, count, what)
    assert not np.isfinite(ref[0][~kept]).any() and not np.isfinite(ref[1][~kept]).any(), what      # safety: no culled pair has a finite time
    return ref, kept, listed, count


def _conditions(fleet, start, level, lo, hi, ref, kept, what):
    """Completeness against the longdouble statements, and the shares: a pair refused in every query is culled; a pair box-far in every
    query with 1e-6 room is culled; so is a pair each of whose queries is one or the other.  Returns the shares, of all pairs."""
    s = ci.shares(fleet, start, level, lo, hi)
    assert not kept[s["refused"]].any(), what
    assert not kept[s["far"]].any(), what
    assert not kept[s["out"]].any(), what
    assert not np.isfinite(ref[0][s["out"]]).any(), what      # the reference's own consistency: such a pair has no time
    finite = np.isfinite(ref[0]).any(axis=2)
    assert kept[finite].all(), what
    out = {name: float(x.mean()) for name, x in s.items()}
    out["finite"], out["culled"] = float(finite.mean()), float((~kept).mean())
    return out


# ---------------------------------------------------------------- 1. forward
def test_forward_is_the_unculled_entry_bit_for_bit(shape, d):
    m, n, ks, _ = SHAPES[shape]
    d = int(d)
    first, second = pairs_of(m)
    small = shape != "64x1"
    for k in ks:
        for spread in ci.SPREADS:
            fleet, start, lo, hi, both = ci.family(n, m, d, k, spread)
            for layout, level in both.items():
                what = (shape, d, k, spread, layout)
                ref, kept, listed, count = _same_as_unculled(fleet, start, level, lo, hi, what)
                s = _conditions(fleet, start, level, lo, hi, ref, kept, what)
                print("%s d = %d k = %d spread %g, level %s: %d queries the same bits in time, local time and rate; %d of %d pairs searched; of the "
                      "pairs, refused %.1f %%, far %.1f %%, either per query %.1f %%, culled %.1f %%, with a finite time %.1f %%"
                      % (shape, d, k, spread, layout, ref[0].size, count, kept.size, 100 * s["refused"], 100 * s["far"], 100 * s["out"],
                         100 * s["culled"], 100 * s["finite"]))
                assert s["refused"] >= ci.REFUSED_LEAST[spread], what
                assert s["finite"] >= ci.finite_least(shape, d, spread), what
                if k == 7:
                    assert s["culled"] - max(s["refused"], s["far"]) >= ci.gain_least(shape, d, spread), what
                if shape != "5x30" or k != 7:
                    continue
                # every pattern of outputs but none; NULL window ends; NULL end velocities: each the un-culled entry's bits
                for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                             (False, True, True)):
                    _, kept_w, _, _ = _same_as_unculled(fleet, start, level, lo, hi, what, want=want, reference=ref)
                    assert np.array_equal(kept_w, kept), what
                _same_as_unculled(fleet, start, level, None, hi, what)
                _same_as_unculled(fleet, start, level, lo, None, what)
                _same_as_unculled(fleet, start, level, None, None, what)
                still = [[x.copy() for x in axis] for axis in fleet]
                for axis in still:
                    axis[3][:], axis[4][:] = 0.0, 0.0
                assert _all_same(_same_as_unculled(still, start, level, lo, hi, what, zero_vel=True)[0], sc._rdv(still, start, level, lo, hi))
                # poisoned starts: exactly those vehicles' pairs NaN, every one of them kept (the search makes their NaNs)
                bad, poisoned = sc._poison(start, ref[0].shape, k)
                got_bad, kept_bad, _, _ = _same_as_unculled(fleet, bad, level, lo, hi, what)
                assert np.array_equal(np.isnan(got_bad[0]), poisoned | np.isnan(ref[0])), what
                assert kept_bad[poisoned.all(axis=2)].all(), what
                # bad durations: the NaN rule; the total is NaN, so `whole` fails and the query is refused: those pairs are culled
                broken, hit = sc._bad_durations(fleet, ref[0].shape, d)
                got_broken, kept_broken, _, _ = _same_as_unculled(broken, start, level, lo, hi, what)
                assert np.array_equal(np.isnan(got_broken[0]), hit | np.isnan(ref[0])), what
                assert not kept_broken[hit.all(axis=2)].any(), what
                if layout != "per scene":
                    continue
                # spoilt levels: NaN, +inf, -inf are refused in that query (finite(level) fails); -1 is a level like any other
                spoilt = level.copy()
                for s_, q, value in ((2, 0, np.nan), (11, 3, np.inf), (20, 6, -1.0), (29, 6, -np.inf)):
                    spoilt[s_, q] = value
                ref_spoilt, kept_spoilt, _, _ = _same_as_unculled(fleet, start, spoilt, lo, hi, what)
                assert np.isnan(ref_spoilt[0][2, :, 0]).all() and np.isnan(ref_spoilt[0][11, :, 3]).all() and np.isnan(ref_spoilt[0][29, :, 6]).all()
                assert not kept_spoilt[ci.shares(fleet, start, spoilt, lo, hi)["out"]].any(), what
    assert small or m == 64


# ---------------------------------------------------------------- 2. the sieve's answer
def _reach(fleet, start, lo, hi, k):
    """rp_trajectory_fleet_reach_staggered: (box_min, box_max), d arrays of (n, m, k) each."""
    n, m = start.shape
    d = len(fleet)
    tf = [[_t(x) for x in axis] for axis in fleet]
    ts, tl, th = (_t(x) if x is not None else None for x in (start, lo, hi))
    outs = [[Out(n, m, k) for _ in range(d)] for _ in range(2)]
    capi.trajectory_fleet_reach_staggered(0, 0, n, m, k, d, [t.data_ptr() for axis in tf for t in axis], ts.data_ptr(),
                                          *[t.data_ptr() if t is not None else 0 for t in (tl, th)], [o.ptr for o in outs[0]],
                                          [o.ptr for o in outs[1]])
    torch.cuda.synchronize()
    return [[o.get() for o in side] for side in outs]


def _extrema(fleet, start, lo, hi, k):
    """rp_trajectory_extrema's pos_min and pos_max on the n m splines of each axis with vehicle v's window [lo - s_v, hi - s_v], formed
    here in float64 (a NULL end: the infinity before the subtraction)."""
    n, m = start.shape
    with np.errstate(all="ignore"):
        shifted = [np.ascontiguousarray(((w if w is not None else np.full((n, k), inf))[:, None, :] - start[:, :, None]).reshape(n * m, k))
                   for w, inf in ((lo, -np.inf), (hi, np.inf))]
    tl, th = _t(shifted[0]), _t(shifted[1])
    out = [[], []]
    for axis in fleet:
        ts = [_t(x.reshape(-1)) for x in axis]
        low, high = Out(n, m, k), Out(n, m, k)
        capi.trajectory_extrema(0, 0, n * m, k, [t.data_ptr() for t in ts], tl.data_ptr(), th.data_ptr(), [low.ptr, high.ptr, 0, 0], None)
        torch.cuda.synchronize()
        out[0].append(low.get())
        out[1].append(high.get())
    return out


def test_the_sieves_answer(shape, d):
    m, n, ks, _ = SHAPES[shape]
    d, k = int(d), (1 if shape == "64x1" else 7)
    for spread in ci.SPREADS:
        fleet, start, lo, hi, both = ci.family(n, m, d, k, spread)
        # the boxes: rp_trajectory_extrema's bits on the n m splines over the shifted windows, with both ends, one and none
        for wl, wh in ((lo, hi), (None, hi), (lo, None), (None, None)):
            kk = k if (wl is not None or wh is not None) else 1
            assert all(_all_same(x, y) for x, y in zip(_reach(fleet, start, wl, wh, kk), _extrema(fleet, start, wl, wh, kk))), (shape, d)
        six = [_t(np.stack([axis[f] for axis in fleet], axis=2)) for f in range(8)]
        box_min, box_max = rp.trajectory_fleet_reach([six[f] for f in SIX], _t(lo), _t(hi), start=_t(start))
        want_min, want_max = _reach(fleet, start, lo, hi, k)
        assert box_min.shape == box_max.shape == (n, m, k, d) and not box_min.requires_grad
        assert _same_bits(box_min.cpu().numpy(), np.stack(want_min, axis=3)) and _same_bits(box_max.cpu().numpy(), np.stack(want_max, axis=3))
        for layout, level in both.items():
            what = (shape, d, spread, layout)
            ref, kept, listed, count = _same_as_unculled(fleet, start, level, lo, hi, what)
            _conditions(fleet, start, level, lo, hi, ref, kept, what)
            again = _culled(fleet, start, level, lo, hi)      # the same list and bits in two runs
            assert _all_same(again[0], ref) and np.array_equal(again[1], kept) and np.array_equal(again[2], listed) and again[3] == count
            flags = rp.fleet_contact_candidates([six[f] for f in SIX], None, _t(lo), _t(hi), level_sq=_t(level), start=_t(start))
            assert flags.dtype == torch.bool and flags.shape == kept.shape and np.array_equal(flags.cpu().numpy(), kept), what
            print("%s d = %d spread %g, level %s: %d of %d pairs kept; the boxes are the extrema entry's bits; the flags, the list and the count "
                  "agree and repeat" % (shape, d, spread, layout, count, kept.size))


# ---------------------------------------------------------------- 3. hand-made scenes
def test_hand_made_scenes():
    for base in (0.0, 2.0 ** 40):
        fleet, start, level, want_refused = ci.touching_scenes(base)
        assert np.array_equal(ci.refused(fleet, start, level, None, None)[:, 0, 0], want_refused)
        ref, kept, _, _ = _same_as_unculled(fleet, start, level, None, None, ("touching", base))
        # the one instant: the end of vehicle i's time, T_i = 2 on its clock, base + 2 on the scene's; kept.  One ulp later: culled
        assert ref[1][0, 0, 0] == 2.0 and ref[0][0, 0, 0] == base + 2.0 and kept[0, 0]
        assert np.isnan(ref[0][1, 0, 0]) and not kept[1, 0]
        assert np.isfinite(ref[0][2, 0, 0]) and kept[2, 0]
        print("touching domains, starts from %g: local times %s, kept %s" % (base, ref[1][:, 0, 0].tolist(), kept[:, 0].astype(int).tolist()))
    fleet, start, level = ci.passing_scenes()
    assert start[0, 1] - start[0, 0] != 0.2
    for lo, hi in ((None, None), (np.full((2, 1), 0.15), np.full((2, 1), 3.7))):
        ref, kept, _, _ = _same_as_unculled(fleet, start, level, lo, hi, "passing")
        assert ref[1][0, 0, 0] == 2.0 and kept[0, 0]      # at exactly the radius at the last instant of vehicle 0: found, so kept
        assert np.isnan(ref[0][1, 0, 0])                   # at r (1 + 2^-40): never at the level
        print("ending at the radius: local times %s, kept %s" % (ref[1][:, 0, 0].tolist(), kept[:, 0].astype(int).tolist()))


# ---------------------------------------------------------------- 4. a list beyond the first trip of the search
def test_past_the_first_trip():
    """m = 3, n = 100,001: 300,003 problems.  The starts are spread over half the shortest total time, so that nearly every pair has a common
    time; in every 21st scene vehicle 2 starts 100 later: its two pairs are refused, and the list positions behind them are no longer the
    problems' numbers.  The list is longer than 2,048 x 128 = 262,144: blocks of the search go on a second trip."""
    m, n, d, k = 3, 100001, 2, 1
    fleet = ci.fleet_inputs(n, m, d)
    start = si.starts_of(fleet, 0.5)
    start[::21, 2] += 100.0
    level = np.full((n, k), 9.0)
    ref, kept, listed, count = _same_as_unculled(fleet, start, level, None, None, "past the first trip")
    late = np.zeros((n, 3), dtype=bool)
    late[::21, 1:] = True
    assert not kept[late].any() and np.isnan(ref[0][late]).all()
    assert 262145 <= count < n * 3, count
    assert np.isfinite(ref[0].reshape(-1)[listed[262144:]]).any()      # times found on the second trip
    print("300,003 problems, %d listed, %d culled: every bit the un-culled entry's; %.1f %% of the queries finite"
          % (count, n * 3 - count, 100 * np.isfinite(ref[0]).mean()))


# ---------------------------------------------------------------- 5. torch
def test_torch_staggered_broad_phase_is_the_same_bits():
    m, n, d, k = 5, 30, 2, 7
    pairs = m * (m - 1) // 2
    fleet, start_np, lo_np, hi_np, both = ci.family(n, m, d, k, 2.0)
    rng = np.random.default_rng(979)
    g = _t(rng.standard_normal((n, pairs, k)))
    lo, hi = _t(lo_np), _t(hi_np)
    for layout, level_np in both.items():
        for by_radius in (False, True):
            leaves = fg._fleet_leaves(fleet)
            start = _t(start_np).requires_grad_()
            query = _t(np.sqrt(level_np) if by_radius else level_np).requires_grad_()
            run = lambda xs, s, q, on: rp.trajectory_fleet_contact([xs[f] for f in SIX], q if by_radius else None, lo, hi,      # noqa: E731
                                                                   level_sq=None if by_radius else q, start=s, broad_phase=on)
            off, on = run(leaves, start, query, False), run(leaves, start, query, "staggered")
            assert on.shape == (n, pairs, k) and on.requires_grad
            assert _same_bits(on.detach().cpu().numpy(), off.detach().cpu().numpy()), (layout, by_radius)
            finite = float(torch.isfinite(off.detach()).any(dim=2).double().mean())
            assert finite >= 0.05, finite
            every = leaves + [start, query]
            want = torch.autograd.grad(off, every, grad_outputs=g)
            got = torch.autograd.grad(on, every, grad_outputs=g)
            assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(got, want)), (layout, by_radius)
            assert float(got[8].abs().max()) > 0      # the starts' own gradient
            dots = [_t(rng.standard_normal((n, m, d))) for _ in range(8)] + [_t(rng.standard_normal((n, m))), _t(rng.standard_normal(level_np.shape))]
            tangents = []
            for flag in (False, "staggered"):
                with fwAD.dual_level():
                    dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(every, dots)]
                    tangents.append(fwAD.unpack_dual(run(dual[:8], dual[8], dual[9], flag)).tangent.cpu().numpy())
            assert _same_bits(tangents[0], tangents[1]), (layout, by_radius)
            assert np.isfinite(tangents[1]).any()
            print('torch, level %s, %s: broad_phase="staggered" gives the same bits in the times, in 10 gradients and in the tangents; %.1f %% '
                  "of the pairs have a finite time" % (layout, "radius=" if by_radius else "level_sq=", 100 * finite))
    kept = rp.fleet_contact_candidates([fg._fleet_leaves(fleet)[f] for f in SIX], None, lo, hi, level_sq=_t(both["per scene"]), start=_t(start_np))
    assert 0.2 <= 1.0 - float(kept.double().mean())      # the option had something to cull
    # through the solves: section 28's pipeline case on golden problems
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
    start_np = si.starts_of(fleet_np, 8.0)
    lo_np, hi_np = si.scene_windows(fleet_np, start_np, k, 970)
    lo, hi = _t(lo_np), _t(hi_np)
    start = _t(start_np).requires_grad_()
    level = _t(sc.levels_of(fleet_np, start_np, lo_np, hi_np, 971)[0])      # one level per pair, as section 28's pipeline case
    outs = [rp.min_time_fleet_contact(x, None, lo, hi, level_sq=level, gap_tol=1e-13, start=start, broad_phase=flag) for flag in (False, "staggered")]
    assert _same_bits(outs[0][0].detach().cpu().numpy(), outs[1][0].detach().cpu().numpy())
    assert float(torch.isfinite(outs[0][0].detach()).double().mean()) >= 0.05
    grads = [[t.cpu().numpy() for t in torch.autograd.grad(torch.nan_to_num(o[0]).sum(), [x[1], start], retain_graph=True)] for o in outs]
    assert _all_same(grads[0], grads[1])
    kept = rp.fleet_contact_candidates(six, None, lo, hi, level_sq=level, start=start.detach())
    print('min_time_fleet_contact(start=, broad_phase="staggered") on the golden problems: the same bits in the times and in d / d pos1 and '
          "d / d start; %.1f %% of the pairs culled, %.1f %% of the queries finite"
          % (100 * (1 - float(kept.double().mean())), 100 * float(torch.isfinite(outs[0][0].detach()).double().mean())))
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
