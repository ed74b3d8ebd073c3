"""The broad phase of the staggered fleet contact query without a GPU (rp_trajectory_fleet_reach_staggered,
rp_trajectory_fleet_contact_staggered_culled(_workspace), rp_trajectory_fleet_contact_staggered_candidates;
trajectory_fleet_contact(start=, broad_phase="staggered"), fleet_contact_candidates(start=), trajectory_fleet_reach(start=); DESIGN.md
section 31): the two tests' arithmetic (csrc/fleet_cull.h) compiled for the host with the address and undefined-behaviour sanitizers into
a stand-alone program (tests/csrc/staggered_cull_check.cpp, which states what it asserts and why) and run as a program; the entries exist
and refuse bad arguments before any device call, the inherited refusals in rp_trajectory_fleet_contact_staggered's order; so does the
torch layer; and the device tests' inputs meet their conditions, by the longdouble statements of tests/staggered_cull_inputs.py alone."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rocket_path_amd as rp
import staggered_cull_inputs as ci
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rp_trajectory_fleet_reach_staggered", "rp_trajectory_fleet_contact_staggered_culled_workspace",
           "rp_trajectory_fleet_contact_staggered_culled", "rp_trajectory_fleet_contact_staggered_candidates")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_two_tests_on_the_host_under_the_sanitizers(tmp_path):
    exe = tmp_path / "staggered_cull_check"
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rocket_path_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "staggered_cull_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = re.findall(r"d=(\d) cases=(\d+) refused=(\d+) far=(\d+) nonfinite=(\d+) timed=(\d+)", r.stdout)
    assert [int(row[0]) for row in rows] == [1, 2, 3]
    for d, cases, refused, far, nonfinite, timed in (tuple(int(x) for x in row) for row in rows):
        assert cases >= 1000000, (d, cases)
        # the statements were asked of something: a good share refused and a good share not, far and not, every non-finite field, and the
        # time error measured on at least a fifth of the cases
        assert refused >= cases // 10 and cases - refused >= cases // 10, (d, refused)
        assert far >= cases // 10 and cases - far >= cases // 10, (d, far)
        assert nonfinite >= 100000, (d, nonfinite)
        assert timed >= cases // 5, (d, timed)


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
        assert callable(getattr(capi, name[3:])), name
    assert "rp_trajectory_fleet_contact_staggered_culled" in header[:header.index("#define RP_ABI_VERSION")]      # in the list of entries
    assert lib.rp_abi_version() == 7      # entries only: the revision stays
    text = header[header.index("with a start time per vehicle (DESIGN.md section 31"):]
    for word in ("bit for bit", "pos_min and pos_max", "lo - start_v", "refused", "far", "exactly once", "NaN or infinite start is kept",
                 "but not all", "no atomics"):
        assert word in text, word


def test_the_workspace_size():
    lib = capi.load_library()
    size = ctypes.c_size_t(7)
    ask, bad = lib.rp_trajectory_fleet_contact_staggered_culled_workspace, capi.RP_ERR_INVALID
    assert ask(30, 5, 7, 2, None) == bad and b"bytes is null" in lib.rp_last_error()
    for m in (1, 257):
        assert ask(30, m, 7, 2, ctypes.byref(size)) == bad and b"m must be 2..256" in lib.rp_last_error() and size.value == 0
    for d in (0, 4):
        assert ask(30, 5, 7, d, ctypes.byref(size)) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error()
    assert ask(0, 5, 7, 2, ctypes.byref(size)) == bad and ask(30, 5, 0, 2, ctypes.byref(size)) == bad
    assert ask(30, 5, 1 << 31, 2, ctypes.byref(size)) == bad and b"2^31" in lib.rp_last_error()
    assert ask(1 << 32, 2, 1, 1, ctypes.byref(size)) == bad and b"2^32" in lib.rp_last_error()
    assert ask((1 << 32) - 1, 2, 1, 1, ctypes.byref(size)) == capi.RP_OK and size.value > 0
    # the boxes (2 d n m k doubles), the slacks, totals and speed bounds (3 d n m), a flag and a list entry per problem, the chunks' counts
    # and the count; the slack: each of the 5 d + 4 parts rounded up to 16 bytes
    for n, m, k, d in ((30, 5, 7, 2), (1, 2, 1, 1), (2, 256, 8, 3), (43, 3, 7, 1)):
        got = capi.trajectory_fleet_contact_staggered_culled_workspace(n, m, k, d)
        problems = n * m * (m - 1) // 2
        least = 8 * (2 * d * n * m * k + 3 * d * n * m) + 5 * problems + 4
        assert got % 16 == 0 and least <= got <= least + 16 * (5 * d + 4) + 4 * (problems // 2048 + 1), (n, m, k, d, got, least)
        assert got == capi.trajectory_fleet_contact_culled_workspace(n, m, k, d) + 2 * d * ((8 * n * m + 15) // 16 * 16)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID
    g = vp(good)
    plenty = 1 << 40
    culled, candidates = lib.rp_trajectory_fleet_contact_staggered_culled, lib.rp_trajectory_fleet_contact_staggered_candidates
    reach = lib.rp_trajectory_fleet_reach_staggered
    for d in (1, 2, 3):
        table = capi.axes_table([good] * (8 * d), d)
        outs = (vp * d)(*[good] * d)
        tail = (g, plenty, g, g, g)
        none = (None, 0, None, None, None)
        for per_pair in (0, 1):
            # rp_trajectory_fleet_contact_staggered's refusals, in its order, ahead of the workspace's (here NULL)
            for m in (1, 0, 257, 1 << 40):
                assert culled(0, None, 4, m, 4, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"m must be 2..256" in lib.rp_last_error()
            assert culled(0, None, 0, 3, 4, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"positive" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 0, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"positive" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 1 << 31, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"2^31" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, None, g, g, per_pair, g, g, g, g, g, *none) == bad and b"d_fleet is null" in lib.rp_last_error()
            assert culled(-1, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"device" in lib.rp_last_error()
            assert culled(0, None, (1 << 63) // 4, 256, 4, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad
            assert b"does not fit" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, None, g, per_pair, g, g, g, g, g, *none) == bad and b"d_start is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, None, per_pair, g, g, g, g, g, *none) == bad and b"d_level_sq is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, None, None, None, *tail) == bad and b"no output" in lib.rp_last_error()
            for at in range(3):      # each output misaligned in turn
                three = [g, g, g]
                three[at] = vp(odd)
                assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, *three, *none) == bad and b"16-byte" in lib.rp_last_error()
            # any output may be left out: the next refusal is then the workspace's
            for three in ((g, None, None), (None, g, None), (None, None, g), (g, g, None), (g, None, g), (None, g, g)):
                assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, *three, *none) == bad and b"d_workspace is null" in lib.rp_last_error()
            # the new ones: the workspace NULL, misaligned, short; n x pairs at 2^32
            assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, g, g, *none) == bad and b"d_workspace is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, g, g, vp(odd), plenty, g, g, g) == bad
            assert b"d_workspace must be 16-byte aligned" in lib.rp_last_error()
            need = capi.trajectory_fleet_contact_staggered_culled_workspace(4, 3, 4, d)
            for short in (0, 16, capi.trajectory_fleet_contact_culled_workspace(4, 3, 4, d), need - 1):
                assert culled(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, g, g, g, short, g, g, g) == bad
                assert b"staggered_culled_workspace asks for" in lib.rp_last_error()
            assert culled(0, None, 1 << 32, 2, 1, d, table, g, g, per_pair, g, g, g, g, g, *tail) == bad and b"2^32" in lib.rp_last_error()
            # the broad phase alone: the same, with the flags required
            assert candidates(0, None, 4, 1, 4, d, table, g, g, per_pair, g, g, g, plenty, g) == bad and b"m must be 2..256" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, None, g, per_pair, g, g, g, plenty, g) == bad and b"d_start is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, None, per_pair, g, g, g, plenty, g) == bad and b"d_level_sq is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, plenty, None) == bad and b"d_kept is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, None, plenty, g) == bad and b"d_workspace is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, g, per_pair, g, g, g, need - 1, g) == bad and b"asks for" in lib.rp_last_error()
        for wrong in (2, -1, 256):
            assert culled(0, None, 4, 3, 4, d, table, g, g, wrong, g, g, g, g, g, *tail) == bad and b"level_per_pair" in lib.rp_last_error(), wrong
        assert culled(0, None, 4, 3, 4, d, table, g, vp(odd), 1, g, g, g, g, g, *tail) == bad and b"16-byte" in lib.rp_last_error()
        # the boxes: rp_trajectory_fleet_reach's refusals in its order, then the start
        for m in (1, 257):
            assert reach(0, None, 4, m, 4, d, table, g, g, g, outs, outs) == bad and b"m must be 2..256" in lib.rp_last_error()
        assert reach(-1, None, 4, 3, 4, d, table, g, g, g, outs, outs) == bad and b"device" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, None, g, g, g, outs, outs) == bad and b"d_fleet is null" in lib.rp_last_error()
        assert reach(0, None, 0, 3, 4, d, table, g, g, g, outs, outs) == bad and b"positive" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 1 << 31, d, table, g, g, g, outs, outs) == bad and b"2^31" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, g, None, None) == bad and b"no output" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, g, (vp * d)(*[odd] * d), None) == bad and b"16-byte" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, None, g, g, outs, outs) == bad and b"d_start is null" in lib.rp_last_error()
    big = capi.axes_table([good] * 32, 4)
    for d in (0, 4, -1):      # before the table is looked at
        assert culled(0, None, 4, 3, 4, d, big, g, g, 0, g, g, g, g, g, g, plenty, g, g, g) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        assert reach(0, None, 4, 3, 4, d, big, g, g, g, None, None) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_contact_staggered_culled(0, 0, 4, 3, 4, d, [good] * 8, good, good, 0, good, good, good, good, good, good, plenty)
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_contact_staggered_culled_workspace(4, 3, 4, d)
    for m in (1, 257):
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_contact_staggered_candidates(0, 0, 4, m, 4, 2, [good] * 16, good, good, 0, good, good, good, plenty, good)
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_reach_staggered(0, 0, 4, m, 4, 2, [good] * 16, good, good, good, [good] * 2, [good] * 2)
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact_staggered_culled(0, 0, 4, 3, 4, 2, [good] * 16, good, good, 0, good, good, good, good, good)      # no workspace
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact_staggered_culled_workspace(1 << 32, 2, 1, 1)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    x = f64(4, 3, 2)      # n = 4 scenes of m = 3 vehicles (3 pairs) in d = 2 axes
    for who, fleet in ((rp.trajectory_fleet_contact, [x] * 6), (rp.min_time_fleet_contact, [x] * 3)):
        # the old refusal stands, and names the new spelling
        with pytest.raises(ValueError, match="broad_phase=True does not take start=.*staggered"):
            who(fleet, f64(4, 5), start=f64(4, 3), broad_phase=True)
        # "staggered" needs start=; any other string is refused: before anything else is looked at, and before any device call
        with pytest.raises(ValueError, match='broad_phase="staggered" needs start='):
            who(fleet, f64(4, 5), broad_phase="staggered")
        with pytest.raises(ValueError, match="broad_phase must be False, True or"):
            who(fleet, f64(4, 5), start=f64(4, 3), broad_phase="boxes")
        with pytest.raises(TypeError, match="either radius or level_sq"):
            who(fleet, start=f64(4, 3), broad_phase="staggered")
        # with the option the checks are the staggered call's, shapes and types before devices
        for wrong in (f64(4), f64(4, 3, 1), f64(12), f64(3, 4)):
            with pytest.raises(ValueError, match="start must have shape"):
                who(fleet, f64(4, 5), start=wrong, broad_phase="staggered")
        with pytest.raises(TypeError, match="float64"):
            who(fleet, f64(4, 5), start=f64(4, 3).float(), broad_phase="staggered")
        with pytest.raises(ValueError, match="radius must have shape"):
            who(fleet, f64(4, 4, 5), start=f64(4, 3), broad_phase="staggered")
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_fleet_contact([x] * 6, f64(4, 5), start=f64(4, 3), broad_phase="staggered")
    cand, reach = rp.fleet_contact_candidates, rp.trajectory_fleet_reach
    for who in (lambda **kw: cand([x] * 6, f64(4, 5), **kw), lambda **kw: reach([x] * 6, f64(4, 5), **kw)):
        for wrong in (f64(4), f64(4, 3, 1), f64(12), f64(3, 4)):
            with pytest.raises(ValueError, match="start must have shape"):
                who(start=wrong)
        with pytest.raises(TypeError, match="float64"):
            who(start=f64(4, 3).float())
        with pytest.raises(TypeError, match="ROCm device"):      # CPU tensors: after every check of shape and type
            who(start=f64(4, 3))
    with pytest.raises(ValueError, match="lo must have shape"):
        reach([x] * 6, f64(3, 5), start=f64(4, 3))
    with pytest.raises(ValueError, match="queries per scene"):
        cand([x] * 6, f64(4, 5), f64(4, 6), start=f64(4, 3))


# ---------------------------------------------------------------- the device tests' inputs
@pytest.mark.parametrize("shape", sorted(ci.SHAPES))
def test_the_device_tests_inputs_meet_their_conditions(shape):
    """By the longdouble statements alone: at spread 8 at least 10 % of the pairs are refused in every query, at spread 2 at least 2 %; at
    k = 7 the pairs out by either test per query exceed the larger single test's share by gain_least; no vehicle has a NaN box under a
    query that is not refused; and the float64 restatement of the refused test -- the search's own operations -- agrees with longdouble on
    every query, so `a pair refused in longdouble is culled` asks nothing that rounding could take away."""
    m, n, ks, ds = ci.SHAPES[shape]
    for d in ds:
        for k in sorted(set(ks) | {7}):      # (64x1 runs k = 1 on the device; its k = 7 is measured here all the same)
            for spread in ci.SPREADS:
                fleet, start, lo, hi, both = ci.family(n, m, d, k, spread)
                for layout, level in both.items():
                    what = (shape, d, k, spread, layout)
                    s = {name: float(v.mean()) for name, v in ci.shares(fleet, start, level, lo, hi).items()}
                    print("%s d = %d k = %d spread %g level %s: refused %.3f, far %.3f, either per query %.3f" % (what + (s["refused"], s["far"], s["out"])))
                    assert s["refused"] >= ci.REFUSED_LEAST[spread], what
                    if k == 7:
                        assert s["out"] - max(s["refused"], s["far"]) >= ci.gain_least(shape, d, spread), what
                        assert s["out"] - max(s["refused"], s["far"]) >= ci.GAIN_MEASURED[(shape, d, spread)] - 0.0015, what      # the table is right (to 0.1 %)
                    assert np.array_equal(ci.refused(fleet, start, level, lo, hi, np.float64), ci.refused(fleet, start, level, lo, hi)), what
                    assert ci.nan_box_under_a_live_query(fleet, start, level, lo, hi) == 0, what


def test_the_hand_made_scenes_are_what_they_say():
    for base in (0.0, 2.0 ** 40):
        fleet, start, level, want = ci.touching_scenes(base)
        for T in (np.longdouble, np.float64):
            assert np.array_equal(ci.refused(fleet, start, level, None, None, T)[:, 0, 0], want), (base, T)
        assert start[0, 1] - start[0, 0] == 2.0 and start[1, 1] - start[1, 0] > 2.0 and start[2, 1] - start[2, 0] < 2.0
    fleet, start, level = ci.passing_scenes()
    assert start[0, 1] - start[0, 0] != 0.2 and not ci.refused(fleet, start, level, None, None).any()
    # the runner ends at x = 0, 4 and 4 (1 + 2^-40) from the two standing vehicles: not far in longdouble at the radius
    assert not ci.far(fleet, start, level, None, None, room=0.0)[0, 0, 0] and ci.far(fleet, start, level, None, None, room=0.0)[1, 0, 0]
