"""The cases of tests/test_gpu_shortlist.py, each run in a fresh process (`python tests/shortlist_gpu_cases.py <case> [arguments]`), on top
of tests/fleet_cull_gpu_cases.py's culled entry with its guards and tests/shortlist_patterns.py's inputs.  Not collected by pytest (no test_
prefix on the file).  What is checked, and why: DESIGN.md section 30, "The shortlist under chosen flags".  Standing vehicles and a level
per pair: 1 is provably out of reach (culled); 400 is kept, and a pair 20 apart is at it at the window's start; NaN is kept and searched
to a NaN.  So
the flags k_shortlist_count, _scan and _scatter see are chosen one by one: the list must be numpy's flatnonzero of the pattern, the count
its sum, and every bit of time and rate the un-culled entry's on the same inputs -- the window's start where the level is 400 and the
pair 20 apart, NaN elsewhere."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_cull_gpu_cases as fu  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fleet_contact_gpu_cases as fc  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import shortlist_patterns as sp  # noqa: E402
import trajectory_gpu_cases as tg  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

_t, _same_bits, SIX = fu._t, fu._same_bits, fu.SIX


def _run(fleet, level, lo, hi, keep, what):
    """The culled entry on inputs made to keep exactly `keep` (n, pairs): fleet_cull_gpu_cases._same_as_unculled's statements -- every bit of
    time and rate the un-culled entry's, nothing left at the sentinel, the guards behind the workspace, the flags, the list and the count
    untouched, the list the flags' indices --, and the flags, the list and the count against numpy on the pattern."""
    want, kept, listed, count = fu._same_as_unculled(fleet, level, lo, hi, what)
    assert np.array_equal(kept, keep), (what, "the flags", int((kept != keep).sum()))
    assert np.array_equal(listed, np.flatnonzero(keep.reshape(-1))), (what, "the list")
    assert count == int(keep.sum()), (what, "the count", count, int(keep.sum()))
    return want


def _standing(n, m, k=1):
    fleet = sp.standing_fleet(n, m)
    lo, hi = sp.windows(n, k)
    return fleet, lo, hi


# ---------------------------------------------------------------- 1. the patterns
def test_patterns(*sizes):
    """m = 2 (the vehicles 20 apart), d = 1, k = 1: problem = scene."""
    for n in (int(x) for x in sizes):
        assert n in sp.SIZES
        fleet, lo, hi = _standing(n, 2)
        chunks, each, share = sp.scan_share(n)
        for name in (sp.AT_THE_LARGEST if n in sp.LARGEST else sp.PATTERNS):
            keep = sp.pattern(name, n)[:, None]
            level = np.ascontiguousarray(sp.levels_of(keep)[:, :, None])
            want = _run(fleet, level, lo, hi, keep, (n, name))
            assert np.array_equal(want[0], sp.expected_times(level, lo, 2), equal_nan=True), (n, name, "the window's start at 400, NaN elsewhere")
            print("%d problems (%d chunks, %d a scan thread, %d threads idle), %s: %d kept; the list, the count and every bit agree"
                  % (n, chunks, each, int((share == 0).sum()), name, int(keep.sum())))


def test_three_vehicles():
    """m = 3, vehicles at 0, 10 and 20: a scene's three pairs straddle threads' eights and chunks; at the level 400 pair (0, 2) is exactly
    at the radius and the other two, 10 apart, are kept and never at it: NaN."""
    for problems in (9, 2049, 4101, 524289):
        n = problems // 3
        assert 3 * n == problems and problems in sp.SIZES
        fleet, lo, hi = _standing(n, 3)
        for name in (sp.AT_THE_LARGEST if problems > 4101 else sp.PATTERNS):
            keep = sp.pattern(name, problems).reshape(n, 3)
            level = np.ascontiguousarray(sp.levels_of(keep)[:, :, None])
            want = _run(fleet, level, lo, hi, keep, (problems, "m = 3", name))
            assert np.array_equal(want[0], sp.expected_times(level, lo, 3), equal_nan=True), (problems, name)
        print("m = 3, %d problems: the list, the count and every bit agree" % problems)


def test_two_queries():
    """k = 2 with the levels (1, 400), (400, 1), (1, 1), (400, 400) in turn: only (1, 1) is culled, and a kept pair gets one time and one
    NaN at its own place."""
    turn = np.array([[sp.CULLED, sp.CONTACT], [sp.CONTACT, sp.CULLED], [sp.CULLED, sp.CULLED], [sp.CONTACT, sp.CONTACT]])
    for n in (9, 2049, 4101, 524289):
        fleet, lo, hi = _standing(n, 2, k=2)
        level = np.ascontiguousarray(turn[np.arange(n) % 4][:, None, :])
        keep = (np.arange(n) % 4 != 2)[:, None]
        want = _run(fleet, level, lo, hi, keep, (n, "k = 2"))
        assert np.array_equal(want[0], sp.expected_times(level, lo, 2), equal_nan=True), n
        print("k = 2, %d problems: %d kept; the list, the count and every bit agree" % (n, int(keep.sum())))


# ---------------------------------------------------------------- 2. the shortlisted search's own second trip
def test_the_shortlists_second_trip():
    """300,001 problems, every 64th culled: 295,313 listed, so k_shortlisted's blocks start a second trip at list position 262,144, which
    is not that problem's number.  A vehicle approaches a standing one at its scene's own speed and the level is the pair's own, so a
    time is its own problem's and no other's.  Every bit is the un-culled entry's; and the problems at trajectory_gpu_cases.GRID_ROWS of
    the list, run as a batch of their own, give the same bits."""
    n = sp.SECOND_TRIP_N
    keep = sp.second_trip_keep()[:, None]
    fleet, speed = sp.approaching_fleet(n)
    level = sp.approaching_levels(keep[:, 0])
    lo, hi = np.zeros((n, 1)), np.full((n, 1), 0.5)
    want = _run(fleet, level, lo, hi, keep, "the second trip")
    listed = np.flatnonzero(keep[:, 0])
    assert len(listed) == 295313 and len(listed) > 2048 * 128 and listed[2048 * 128] != 2048 * 128
    assert np.isfinite(want[0][keep[:, 0]]).all() and np.isnan(want[0][~keep[:, 0]]).all()
    # the plain expectation: the distance r is reached at (10 - r) / v.  The search and the square root are good to some 1e-15; neighbouring
    # problems' times differ by some 0.1, and 1e-9 only has to tell a problem's own time from another's
    reach = (sp.APART - np.sqrt(level[:, 0, 0])) / speed
    assert np.all(np.abs(want[0][keep[:, 0], 0, 0] - reach[keep[:, 0]]) <= 1e-9), float(np.nanmax(np.abs(want[0][:, 0, 0] - reach)))
    for rows in tg.GRID_ROWS[:2] + (slice(len(listed) - 257, len(listed)),):
        own = listed[rows]
        time, rate, kept, own_list, count = fu._culled(fc._scenes(fleet, own), np.ascontiguousarray(level[own]), lo[own], hi[own])
        assert kept.all() and count == len(own) and np.array_equal(own_list, np.arange(len(own)))
        assert _same_bits(time, want[0][own]) and _same_bits(rate, want[1][own]), rows
    print("the shortlisted search beyond the grid's cap: %d of %d problems listed, every bit the un-culled entry's, and the same in a batch "
          "of their own" % (len(listed), n))


# ---------------------------------------------------------------- 3. the candidates entries
def test_candidates():
    """rp_trajectory_fleet_contact_candidates and fleet_contact_candidates on 524,289 problems (257 chunks): the flags are the pattern."""
    n = 524289
    fleet, lo, hi = _standing(n, 2)
    tf = [[_t(x) for x in axis] for axis in fleet]
    six = [_t(np.stack([axis[f] for axis in fleet], axis=2)) for f in range(8)]
    tl, th = _t(lo), _t(hi)
    size = capi.trajectory_fleet_contact_culled_workspace(n, 2, 1, 1)
    for name in sp.AT_THE_LARGEST:
        keep = sp.pattern(name, n)[:, None]
        level = _t(sp.levels_of(keep)[:, :, None])
        work = torch.full((size + 64,), 0x5A, dtype=torch.uint8, device=tl.device)
        kept = torch.full((n + fu.GUARD,), fu.FLAG_GUARD, dtype=torch.uint8, device=tl.device)
        torch.cuda.synchronize()
        capi.trajectory_fleet_contact_candidates(0, 0, n, 2, 1, 1, [t.data_ptr() for axis in tf for t in axis], level.data_ptr(), 1, tl.data_ptr(),
                                                 th.data_ptr(), work.data_ptr(), size, kept.data_ptr())
        torch.cuda.synchronize()
        assert bool((work[size:] == 0x5A).all()), "the bytes behind the workspace were written"
        kept = kept.cpu().numpy()
        assert np.all(kept[n:] == fu.FLAG_GUARD) and np.array_equal(kept[:n].reshape(n, 1), keep.astype(np.uint8)), name
        flags = rp.fleet_contact_candidates([six[f] for f in SIX], None, tl, th, level_sq=level)
        assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), keep), name
        print("the candidates entries, %d problems, %s: the flags are the pattern" % (n, name))


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
