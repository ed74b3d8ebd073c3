"""The broad phase of the fleet contact query without a GPU (rp_trajectory_fleet_reach, rp_trajectory_fleet_contact_culled(_workspace),
rp_trajectory_fleet_contact_candidates; trajectory_fleet_contact(broad_phase=True), fleet_contact_candidates, trajectory_fleet_reach;
DESIGN.md section 30): the bound's arithmetic (csrc/fleet_cull.h) compiled for the host with the address and undefined-behaviour sanitizers
into a stand-alone program (tests/csrc/fleet_cull_check.cpp, which states what it asserts and why) and run as a program; the entries exist
and refuse bad arguments before any device call, the inherited refusals in rp_trajectory_fleet_contact's order; and so does the torch
layer."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import rocket_path_amd as rp
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rp_trajectory_fleet_reach", "rp_trajectory_fleet_contact_culled_workspace", "rp_trajectory_fleet_contact_culled",
           "rp_trajectory_fleet_contact_candidates")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_bound_on_the_host_under_the_sanitizers(tmp_path):
    exe = tmp_path / "fleet_cull_check"
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rocket_path_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "fleet_cull_check.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = re.findall(r"d=(\d) cases=(\d+) far=(\d+) nonfinite=(\d+) third=(\d+)", r.stdout)
    assert [int(row[0]) for row in rows] == [1, 2, 3]
    for d, cases, far, nonfinite, third in (tuple(int(x) for x in row) for row in rows):
        assert cases >= 1000000, (d, cases)
        # the statements were asked of something: a good share far, a good share kept, every non-finite field, and the third statement's
        # conditions met by at least a tenth of the cases
        assert far >= cases // 10 and cases - far >= cases // 10, (d, far)
        assert nonfinite >= 100000, (d, nonfinite)
        assert third >= cases // 10, (d, third)


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
        assert callable(getattr(capi, name[3:])), name
    assert "rp_trajectory_fleet_contact_culled" in header[:header.index("#define RP_ABI_VERSION")]      # in the list of entries
    assert lib.rp_abi_version() == 7      # entries only: the revision stays
    text = header[header.index("with a broad phase in front (DESIGN.md section 30"):]
    for word in ("bit for bit", "pos_min and pos_max", "16-byte aligned", "exactly once", "2^32", "increasing order", "waits for another",
                 "no atomics"):
        assert word in text, word
    for name in ("fleet_contact_candidates", "trajectory_fleet_reach"):
        assert getattr(rp, name).__name__ == name


def test_the_workspace_size():
    lib = capi.load_library()
    size = ctypes.c_size_t(7)
    ask, bad = lib.rp_trajectory_fleet_contact_culled_workspace, capi.RP_ERR_INVALID
    assert ask(30, 5, 7, 2, None) == bad and b"bytes is null" in lib.rp_last_error()
    for m in (1, 257):
        assert ask(30, m, 7, 2, ctypes.byref(size)) == bad and b"m must be 2..256" in lib.rp_last_error() and size.value == 0
    for d in (0, 4):
        assert ask(30, 5, 7, d, ctypes.byref(size)) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error()
    assert ask(0, 5, 7, 2, ctypes.byref(size)) == bad and ask(30, 5, 0, 2, ctypes.byref(size)) == bad
    assert ask(30, 5, 1 << 31, 2, ctypes.byref(size)) == bad and b"2^31" in lib.rp_last_error()
    assert ask(1 << 32, 2, 1, 1, ctypes.byref(size)) == bad and b"2^32" in lib.rp_last_error()      # one pair a scene: 2^32 problems
    assert ask((1 << 32) - 1, 2, 1, 1, ctypes.byref(size)) == capi.RP_OK and size.value > 0
    assert ask(131586, 256, 1, 1, ctypes.byref(size)) == capi.RP_OK      # 131,586 x 32,640 = 2^32 - 256
    assert ask(131587, 256, 1, 1, ctypes.byref(size)) == bad and b"2^32" in lib.rp_last_error()
    # the boxes (2 d n m k doubles), the slacks (d n m), a flag and a list entry per problem, the chunks' counts and the count
    for n, m, k, d in ((30, 5, 7, 2), (1, 2, 1, 1), (2, 256, 8, 3), (43, 3, 7, 1)):
        got = capi.trajectory_fleet_contact_culled_workspace(n, m, k, d)
        problems = n * m * (m - 1) // 2
        least = 8 * (2 * d * n * m * k + d * n * m) + 5 * problems + 4
        assert got % 16 == 0 and least <= got <= least + 16 * (3 * d + 4) + 4 * (problems // 2048 + 1), (n, m, k, d, got, least)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID
    g = vp(good)
    plenty = 1 << 40
    culled, candidates, reach = lib.rp_trajectory_fleet_contact_culled, lib.rp_trajectory_fleet_contact_candidates, lib.rp_trajectory_fleet_reach
    for d in (1, 2, 3):
        table = capi.axes_table([good] * (8 * d), d)
        outs = (vp * d)(*[good] * d)
        tail = (g, plenty, g, g, g)
        for per_pair in (0, 1):
            # rp_trajectory_fleet_contact's refusals, in its order, ahead of the workspace's (here NULL)
            none = (None, 0, None, None, None)
            for m in (1, 0, 257, 1 << 40):
                assert culled(0, None, 4, m, 4, d, table, g, per_pair, g, g, g, g, *none) == bad and b"m must be 2..256" in lib.rp_last_error(), m
            assert culled(0, None, 0, 3, 4, d, table, g, per_pair, g, g, g, g, *none) == bad and b"positive" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 0, d, table, g, per_pair, g, g, g, g, *none) == bad and b"positive" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 1 << 31, d, table, g, per_pair, g, g, g, g, *none) == bad and b"2^31" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, None, g, per_pair, g, g, g, g, *none) == bad and b"d_fleet is null" in lib.rp_last_error()
            assert culled(-1, None, 4, 3, 4, d, table, g, per_pair, g, g, g, g, *none) == bad and b"device" in lib.rp_last_error()
            assert culled(0, None, (1 << 63) // 4, 256, 4, d, table, g, per_pair, g, g, g, g, *none) == bad and b"does not fit" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, None, per_pair, g, g, g, g, *none) == bad and b"d_level_sq is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, None, g, *none) == bad and b"d_time is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, vp(odd), g, *none) == bad and b"16-byte" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, vp(odd), *none) == bad and b"every n x k array" in lib.rp_last_error()
            # the new ones: the workspace NULL, misaligned, short; n x pairs at 2^32
            assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, g, *none) == bad and b"d_workspace is null" in lib.rp_last_error()
            assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, g, vp(odd), plenty, g, g, g) == bad
            assert b"d_workspace must be 16-byte aligned" in lib.rp_last_error()
            need = capi.trajectory_fleet_contact_culled_workspace(4, 3, 4, d)
            for short in (0, 16, need - 1):
                assert culled(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, g, g, short, g, g, g) == bad and b"asks for" in lib.rp_last_error()
            assert culled(0, None, 1 << 32, 2, 1, d, table, g, per_pair, g, g, g, g, *tail) == bad and b"2^32" in lib.rp_last_error()
            # the broad phase alone: the same, with the flags required in the time's place
            assert candidates(0, None, 4, 1, 4, d, table, g, per_pair, g, g, g, plenty, g) == bad and b"m must be 2..256" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, None, per_pair, g, g, g, plenty, g) == bad and b"d_level_sq is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, plenty, None) == bad and b"d_kept is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, per_pair, g, g, None, plenty, g) == bad and b"d_workspace is null" in lib.rp_last_error()
            assert candidates(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, need - 1, g) == bad and b"asks for" in lib.rp_last_error()
        for wrong in (2, -1, 256):
            assert culled(0, None, 4, 3, 4, d, table, g, wrong, g, g, g, g, *tail) == bad and b"level_per_pair" in lib.rp_last_error(), wrong
        assert culled(0, None, 4, 3, 4, d, table, vp(odd), 1, g, g, g, g, *tail) == bad and b"16-byte" in lib.rp_last_error()
        # the boxes
        for m in (1, 257):
            assert reach(0, None, 4, m, 4, d, table, g, g, outs, outs) == bad and b"m must be 2..256" in lib.rp_last_error()
        assert reach(-1, None, 4, 3, 4, d, table, g, g, outs, outs) == bad and b"device" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, None, g, g, outs, outs) == bad and b"d_fleet is null" in lib.rp_last_error()
        assert reach(0, None, 0, 3, 4, d, table, g, g, outs, outs) == bad and b"positive" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 0, d, table, g, g, outs, outs) == bad and b"positive" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 1 << 31, d, table, g, g, outs, outs) == bad and b"2^31" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, None, None) == bad and b"no output" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, (vp * d)(), None) == bad and b"no output" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, (vp * d)(*[odd] * d), None) == bad and b"16-byte" in lib.rp_last_error()
        assert reach(0, None, 4, 3, 4, d, table, g, g, None, (vp * d)(*[odd] * d)) == bad and b"16-byte" in lib.rp_last_error()
        entries = [good] * (8 * d)
        entries[8 * (d - 1) + 6] = 0
        assert reach(0, None, 4, 3, 4, d, capi.axes_table(entries, d), g, g, outs, outs) == bad and b"is null" in lib.rp_last_error()
    big = capi.axes_table([good] * 32, 4)
    for d in (0, 4, -1):      # before the table is looked at
        assert culled(0, None, 4, 3, 4, d, big, g, 0, g, g, g, g, g, plenty, g, g, g) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        assert reach(0, None, 4, 3, 4, d, big, g, g, None, None) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_contact_culled(0, 0, 4, 3, 4, d, [good] * 8, good, 0, good, good, good, good, good, plenty)
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_contact_culled_workspace(4, 3, 4, d)
    for m in (1, 257):
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_contact_candidates(0, 0, 4, m, 4, 2, [good] * 16, good, 0, good, good, good, plenty, good)
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_reach(0, 0, 4, m, 4, 2, [good] * 16, good, good, [good] * 2, [good] * 2)
    with pytest.raises(ValueError, match="2 entries"):
        capi.trajectory_fleet_reach(0, 0, 4, 3, 4, 2, [good] * 16, good, good, [good] * 3, None)
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact_culled(0, 0, 4, 3, 4, 2, [good] * 16, good, 0, good, good, good, good)      # no workspace
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact_culled_workspace(1 << 32, 2, 1, 1)


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    x = f64(4, 3, 2)      # n = 4 scenes of m = 3 vehicles (3 pairs) in d = 2 axes
    # broad_phase=True with start=: refused before anything else is looked at, and before any device call (CPU tensors throughout)
    for who, fleet in ((rp.trajectory_fleet_contact, [x] * 6), (rp.min_time_fleet_contact, [x] * 3)):
        with pytest.raises(ValueError, match="broad_phase=True does not take start="):
            who(fleet, f64(4, 5), start=f64(4, 3), broad_phase=True)
        with pytest.raises(TypeError, match="either radius or level_sq"):
            who(fleet, broad_phase=True)
    # with the option the checks are the same ones, shapes and types before devices
    with pytest.raises(TypeError, match="ROCm device"):
        rp.trajectory_fleet_contact([x] * 6, f64(4, 5), broad_phase=True)
    with pytest.raises(ValueError, match="radius must have shape"):
        rp.trajectory_fleet_contact([x] * 6, f64(4, 4, 5), broad_phase=True)
    cand, reach = rp.fleet_contact_candidates, rp.trajectory_fleet_reach
    for radius in (f64(4, 5), f64(5), f64(4, 3, 5)):                    # CPU tensors: after every check of shape and type
        with pytest.raises(TypeError, match="ROCm device"):
            cand([x] * 6, radius)
        with pytest.raises(TypeError, match="ROCm device"):
            cand([x] * 8, None, f64(4, 5), f64(5), level_sq=radius)
    with pytest.raises(TypeError, match="ROCm device"):
        reach([x] * 6)
    with pytest.raises(TypeError, match="ROCm device"):
        reach([x] * 8, f64(4, 5), f64(5))
    with pytest.raises(TypeError, match="either radius or level_sq"):
        cand([x] * 6)
    with pytest.raises(TypeError, match="either radius or level_sq"):
        cand([x] * 6, f64(4, 5), level_sq=f64(4, 5))
    for who in (lambda fleet, *a: cand(fleet, f64(4, 5), *a), reach):
        with pytest.raises(TypeError, match="list or tuple"):
            who(x)
        with pytest.raises(ValueError, match="six"):
            who([x] * 7)
        with pytest.raises(TypeError, match="torch.Tensor"):
            who([x] * 5 + [None])
        for wrong in (f64(4, 2), f64(4), f64(4, 3, 2, 1)):
            with pytest.raises(ValueError, match=r"\(n, m, d\)"):
                who([wrong] * 6)
        for m in (1, 257):
            with pytest.raises(ValueError, match="2..256 vehicles"):
                who([f64(4, m, 2)] * 6)
        for d in (0, 4):
            with pytest.raises(ValueError, match="axes"):
                who([f64(4, 3, d)] * 6)
        with pytest.raises(ValueError, match="duration1 has shape"):
            who([x] * 5 + [f64(4, 2, 2)])
        with pytest.raises(TypeError, match="float64"):
            who([x] * 5 + [x.float()])
        for wrong in (f64(4, 3, 5), f64(3, 5), f64(4, 0), f64(0)):      # a window per scene and query, not per pair
            with pytest.raises(ValueError, match="lo must have shape"):
                who([x] * 6, wrong)
        with pytest.raises(TypeError, match="float64"):
            who([x] * 6, None, torch.zeros(5, dtype=torch.int64))
        with pytest.raises(ValueError, match="lo has shape"):
            who([x] * 6, f64(4, 5), f64(4, 6))
    for wrong in (f64(4, 2, 5), f64(3, 5), f64(4, 0), f64(0), f64(4, 3, 5, 1)):
        with pytest.raises(ValueError, match="radius must have shape"):
            cand([x] * 6, wrong)
        with pytest.raises(ValueError, match="level_sq must have shape"):
            cand([x] * 6, level_sq=wrong)
    with pytest.raises(TypeError, match="float64"):
        cand([x] * 6, torch.zeros((4, 5)))
    with pytest.raises(ValueError, match="queries per scene"):
        cand([x] * 6, f64(4, 5), f64(4, 6))
