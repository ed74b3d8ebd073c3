"""The inputs of the shortlist's device tests without a GPU (tests/shortlist_patterns.py, tests/test_gpu_shortlist.py; DESIGN.md section
30, "The shortlist under chosen flags"): the flag patterns meet the conditions they are named for at every size; the sizes put
k_shortlist_scan's one block where the section says -- 256 chunks with every thread busy, 257 with two chunks a thread and the upper
threads idle, 385 and 518 with a thread that has fewer chunks than its neighbours --; the second-trip case lists more problems than the
grid's cap reaches in one trip; and the scenes are far, or not, at the levels that choose the flags: csrc/fleet_cull.h compiled for the
host with the address and undefined-behaviour sanitizers into a stand-alone program (tests/csrc/shortlist_scene_check.cpp) and run as a
program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shortlist_patterns as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", sp.SIZES)
def test_the_patterns_meet_their_conditions(n):
    chunks = sp.chunks_of(n)
    first, end = sp.middle_chunk(n)
    want = {"nothing": 0, "everything": n, "the first problem": 1, "the last problem": 1, "the first flag of every chunk": chunks,
            "the last flag of every chunk": chunks, "every eighth": n // 8, "one whole chunk": end - first, "all but one whole chunk": n - (end - first)}
    assert set(want) | set(sp.DENSITY) == set(sp.PATTERNS) and set(sp.AT_THE_LARGEST) <= set(sp.PATTERNS)
    per_chunk = lambda keep: np.add.reduceat(keep.astype(np.int64), np.arange(0, n, sp.CHUNK))      # noqa: E731
    for name in sp.PATTERNS:
        keep = sp.pattern(name, n)
        assert keep.shape == (n,) and keep.dtype == bool, name
        assert np.array_equal(keep, sp.pattern(name, n)), name      # the same in every call
        if name in want:
            assert int(keep.sum()) == want[name], (name, int(keep.sum()))
        else:      # six standard deviations of the binomial count, and one for a size of 1
            q = sp.DENSITY[name]
            assert abs(int(keep.sum()) - n * q) <= 6 * np.sqrt(n * q * (1 - q)) + 1, (name, int(keep.sum()))
    assert sp.pattern("the first problem", n)[0] and sp.pattern("the last problem", n)[n - 1]
    size = np.minimum(sp.CHUNK, n - sp.CHUNK * np.arange(chunks))      # flags per chunk: the last one ragged
    firsts, lasts = sp.pattern("the first flag of every chunk", n), sp.pattern("the last flag of every chunk", n)
    assert np.all(per_chunk(firsts) == 1) and np.all(firsts[::sp.CHUNK])
    assert np.all(per_chunk(lasts) == 1) and np.all(lasts[np.cumsum(size) - 1]) and lasts[n - 1]
    eighth = sp.pattern("every eighth", n)
    assert np.all(eighth[7::8]) and int(eighth.sum()) == len(eighth[7::8])      # the last of a thread's eight flags, and no other
    whole, rest = per_chunk(sp.pattern("one whole chunk", n)), per_chunk(sp.pattern("all but one whole chunk", n))
    assert whole[(chunks - 1) // 2] == size[(chunks - 1) // 2] == whole.sum()
    assert np.array_equal(rest, size - whole) and (chunks == 1 or end - first == sp.CHUNK)
    # the levels: every kept flag gets 400 or NaN, both kinds once there are three kept; every other 1
    for name in sp.PATTERNS:
        keep = sp.pattern(name, n)
        level = sp.levels_of(keep)
        assert np.all(level[~keep] == sp.CULLED) and np.all((level[keep] == sp.CONTACT) | np.isnan(level[keep])), name
        assert int(np.isnan(level).sum()) == int(keep.sum()) // 3, name


def test_the_sizes_put_the_scan_where_the_section_says():
    share = {n: sp.scan_share(n) for n in sp.SIZES}
    assert [share[n][0] for n in sp.SIZES] == [1, 1, 1, 1, 1, 1, 2, 3, 256, 257, 385, 518]
    assert [share[n][1] for n in sp.SIZES] == [1] * 9 + [2, 2, 3]
    for n in sp.SIZES:
        chunks, each, mine = share[n]
        assert mine.sum() == chunks and mine.max() == each and np.all(np.diff(mine) <= 0), n
    assert np.all(share[524288][2] == 1)                                                     # every scan thread busy
    mine = share[524289][2]
    assert np.all(mine[:128] == 2) and mine[128] == 1 and np.all(mine[129:] == 0)            # the last chunk alone; threads above 128 idle
    assert 524289 - 256 * sp.CHUNK == 1                                                      # ... and it holds one flag
    mine = share[786437][2]
    assert np.all(mine[:192] == 2) and mine[192] == 1 and np.all(mine[193:] == 0)
    mine = share[1060000][2]
    assert np.all(mine[:172] == 3) and mine[172] == 2 and np.all(mine[173:] == 0)
    assert sp.LARGEST == sp.SIZES[-2:] and max(sp.SIZES) < 1 << 32


def test_the_second_trip_lists_more_than_one_trip_of_the_grid():
    keep = sp.second_trip_keep()
    listed = np.flatnonzero(keep)
    cap = 2048 * 128      # kTrajGridCap blocks of 128 problems
    assert len(keep) == 300001 and len(listed) == 295313 > 262144 == cap
    assert listed[cap] == cap + cap // 63 + 1 != cap      # the second trip's first list position is another problem's number
    fleet, speed = sp.approaching_fleet(len(keep))
    level = sp.approaching_levels(keep)
    assert level.shape == (len(keep), 1, 1) and np.all(level[~keep] == sp.CULLED)
    r = np.sqrt(level[keep, 0, 0])
    gap = sp.APART - 0.5 * speed                     # the boxes' distance over the window [0, 0.5]
    assert np.all(gap >= 9.0) and np.all(r > gap[keep] + 0.05) and np.all((sp.APART - r) / speed[keep] < 0.45)
    assert np.all(fleet[0][2][:, 1] == sp.APART - 2 * speed) and np.all(fleet[0][0][:, 0] == 0)


def test_the_standing_scene_and_its_windows():
    for m in (2, 3):
        fleet = sp.standing_fleet(5, m)
        assert len(fleet) == 1 and all(x.shape == (5, m) for x in fleet[0])
        for f in (0, 1, 2):
            assert np.all(fleet[0][f] == ([0.0, 20.0] if m == 2 else [0.0, 10.0, 20.0]))
        assert all(np.all(fleet[0][f] == 0) for f in (3, 4, 5)) and all(np.all(fleet[0][f] == 1) for f in (6, 7))
    lo, hi = sp.windows(4101, 2)
    assert lo.shape == hi.shape == (4101, 2) and np.all(lo >= 0) and np.all(hi <= 1.5) and np.all(hi - lo == 0.5)
    assert len(np.unique(lo)) > 4000      # a problem's start is its own
    level = np.array([[[sp.CONTACT, sp.CULLED]], [[np.nan, sp.CONTACT]]])
    assert np.array_equal(sp.expected_times(level, lo[:2], 2), [[[lo[0, 0], np.nan]], [[np.nan, lo[1, 1]]]], equal_nan=True)
    level = np.full((2, 3, 2), sp.CONTACT)      # three vehicles: only the pair 20 apart, (0, 2), is ever at 400
    want = np.full((2, 3, 2), np.nan)
    want[:, 1, :] = lo[:2]
    assert np.array_equal(sp.expected_times(level, lo[:2], 3), want, equal_nan=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_scenes_are_far_where_the_levels_say(tmp_path):
    exe = tmp_path / "shortlist_scene_check"
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rocket_path_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "shortlist_scene_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "failures=0" in r.stdout
    rows = re.findall(r"^(standing|approaching).*level (\S+): (far|not far)$", r.stdout, flags=re.M)
    assert len(rows) == 3 * 4 + 5 * 3
    for kind, level, answer in rows:      # the levels that choose the flags: 1 is far, everything else -- 400, NaN, 9.6^2, 9.9^2 -- is not
        assert (answer == "far") == (float(level) == sp.CULLED), (kind, level, answer)
    assert {float(level) for kind, level, _ in rows if kind == "standing" and level != "nan"} == {sp.CULLED, sp.CONTACT}
