"""The fleet queries with a start time per vehicle without a GPU (rp_trajectory_fleet_separation_staggered,
rp_trajectory_fleet_contact_staggered, start= of the four torch functions): the entries exist and refuse bad arguments
before any device call, so does the torch layer -- shapes and types before devices --, and the inputs of the device tests meet the
section's conditions, measured with the float64 restatement of the pair entry (tests/separation_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import rocket_path_amd as rp
import separation_ref as sr
import staggered_inputs as si
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rp_trajectory_fleet_separation_staggered", "rp_trajectory_fleet_contact_staggered")


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in NAMES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header)
        assert name in capi.SIGNATURES and hasattr(lib, name)
        assert name in header[:header.index("#define RP_ABI_VERSION")]      # in the list of entries
        assert callable(getattr(capi, name[3:]))
    text = header[header.index("the two fleet queries with a start time per vehicle"):]
    for word in ("n x m", "s m + v", "delay = s_j - s_i", "lo' = lo - s_i", "bit for bit", "d_time_local", "t' + s_i", "m - 1 pairs",
                 "but not all", "NULL d_start", "No pair-expanded"):
        assert word in text, word
    assert lib.rp_abi_version() == 7      # entries only: the revision stays


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    bad = capi.RP_ERR_INVALID
    g = vp(good)
    sep = lambda device, n, m, k, d, table, start, outs: lib.rp_trajectory_fleet_separation_staggered(device, None, n, m, k, d, table, start, g, g, *outs)      # noqa: E731
    con = lambda device, n, m, k, d, table, start, outs, level=g, per_pair=0: lib.rp_trajectory_fleet_contact_staggered(      # noqa: E731
        device, None, n, m, k, d, table, start, level, per_pair, g, g, *outs)
    all_three = (g, g, g)
    for entry in (sep, con):
        for d in (1, 2, 3):
            table = capi.axes_table([good] * (8 * d), d)
            for m in (1, 0, 257, 1 << 40):
                assert entry(0, 4, m, 4, d, table, g, all_three) == bad and b"m must be 2..256" in lib.rp_last_error(), m
            assert entry(0, 0, 3, 4, d, table, g, all_three) == bad and b"positive" in lib.rp_last_error()
            assert entry(0, 4, 3, 0, d, table, g, all_three) == bad and b"positive" in lib.rp_last_error()
            assert entry(0, 4, 3, 1 << 31, d, table, g, all_three) == bad and b"2^31" in lib.rp_last_error()
            assert entry(0, 4, 3, 4, d, None, g, all_three) == bad and b"d_fleet is null" in lib.rp_last_error()
            assert entry(-1, 4, 3, 4, d, table, g, all_three) == bad
            assert entry(0, (1 << 63) // 4, 256, 4, d, table, g, all_three) == bad and b"does not fit" in lib.rp_last_error()
            assert entry(0, 4, 3, 4, d, table, None, all_three) == bad and b"d_start is null" in lib.rp_last_error()
            for f in range(8 * d):      # the end velocities of any axis may be NULL: those calls fail later, for want of an output
                entries = [good] * (8 * d)
                entries[f] = 0
                assert entry(0, 4, 3, 4, d, capi.axes_table(entries, d), g, (None, None, None)) == bad
                assert (b"no output" in lib.rp_last_error()) == (f % 8 in (3, 4)), (d, f)
            # all outputs NULL; each alone is allowed and gets as far as the alignment; the starts and windows are read as single values
            assert entry(0, 4, 3, 4, d, table, vp(odd), (None, None, None)) == bad and b"no output" in lib.rp_last_error()
            for at in range(3):
                outs = [None] * 3
                outs[at] = vp(odd)
                assert entry(0, 4, 3, 4, d, table, vp(odd), outs) == bad and b"16-byte" in lib.rp_last_error(), at
        big = capi.axes_table([good] * 32, 4)
        for d in (0, 4, -1):      # before the table is looked at
            assert entry(0, 4, 3, 4, d, big, g, all_three) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
    table = capi.axes_table([good] * 16, 2)
    assert con(0, 4, 3, 4, 2, table, g, all_three, level=None) == bad and b"d_level_sq is null" in lib.rp_last_error()
    assert con(0, 4, 3, 4, 2, table, g, all_three, per_pair=2) == bad and b"level_per_pair" in lib.rp_last_error()
    assert con(0, 4, 3, 4, 2, table, g, all_three, level=vp(odd), per_pair=1) == bad and b"16-byte" in lib.rp_last_error()
    # the mirror in capi
    for call, rest in ((capi.trajectory_fleet_separation_staggered, ()), (capi.trajectory_fleet_contact_staggered, (good,))):
        for d in (0, 4):
            with pytest.raises(ValueError, match="d must be"):
                call(0, 0, 4, 3, 4, d, [good] * 8, good, *rest, d_time=good)
        for m in (1, 257):
            with pytest.raises(ValueError, match="m must be"):
                call(0, 0, 4, m, 4, 2, [good] * 16, good, *rest, d_time=good)
        with pytest.raises(ValueError, match="16 entries"):
            call(0, 0, 4, 3, 4, 2, [good] * 8, good, *rest, d_time=good)
        with pytest.raises(rp.RpError):
            call(0, 0, 4, 3, 4, 2, [good] * 16, good, *rest)      # no output
        with pytest.raises(rp.RpError):
            call(0, 0, 4, 3, 4, 2, [good] * 16, None, *rest, d_time=good)      # no start


def test_torch_layer_checks_the_start_before_any_device():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    n, m, d = 4, 3, 2
    x = f64(n, m, d)
    calls = (lambda start, **kw: rp.trajectory_fleet_separation([x] * 6, start=start, **kw),
             lambda start, **kw: rp.trajectory_fleet_contact([x] * 6, f64(n, 5), start=start, **kw),
             lambda start, **kw: rp.min_time_fleet_separation([x] * 3, start=start, **kw),
             lambda start, **kw: rp.min_time_fleet_contact([x] * 3, f64(n, 5), start=start, **kw))
    for call in calls:
        for wrong in (f64(n), f64(n, m, 1), f64(n * m), f64(m, n), f64(n, m + 1)):
            with pytest.raises(ValueError, match=r"start must have shape \(4, 3\)"):
                call(wrong)
        with pytest.raises(TypeError, match="float64"):
            call(torch.zeros((n, m), dtype=torch.float32))
        with pytest.raises(TypeError, match="torch.Tensor"):
            call([[0.0] * m] * n)
        with pytest.raises(TypeError, match="start is on meta; it must be on the fleet's device cpu"):      # another device: after shapes and types
            call(torch.zeros((n, m), dtype=torch.float64, device="meta"))
        with pytest.raises(ValueError, match="hi must have shape"):      # a window's shape before the start's device
            call(torch.zeros((n, m), dtype=torch.float64, device="meta"), hi=f64(n, m, 5))
        with pytest.raises(TypeError, match="ROCm device"):      # CPU tensors: after every check of shape and type
            call(f64(n, m))
        with pytest.raises(TypeError, match="ROCm device"):      # without a start: the call as it was
            call(None)
    for bad_m in (1, 257):
        with pytest.raises(ValueError, match="2..256 vehicles"):
            rp.trajectory_fleet_separation([f64(2, bad_m, 2)] * 6, start=f64(2, bad_m))
        with pytest.raises(ValueError, match="2..256 vehicles"):
            rp.min_time_fleet_contact([f64(2, bad_m, 2)] * 3, f64(2, 5), start=f64(2, bad_m))
    for bad_d in (0, 4):
        with pytest.raises(ValueError, match="axes"):
            rp.trajectory_fleet_contact([f64(4, 3, bad_d)] * 6, f64(4, 5), start=f64(4, 3))
        with pytest.raises(ValueError, match="d in 1..3"):
            rp.min_time_fleet_separation([f64(4, 3, bad_d)] * 3, start=f64(4, 3))


SHAPES = {"5x30": (5, 30), "3x43": (3, 43), "2x300": (2, 300)}      # section 26's, (m, n)


def _fleet_inputs(n, m, d):      # tests/fleet_gpu_cases.py's family
    per = [[tr.random_states(n, 1 + c + 3 * v) for v in range(m)] for c in range(d)]
    return [[np.ascontiguousarray(np.stack([per[c][v][f] for v in range(m)], axis=1)) for f in range(8)] for c in range(d)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_device_tests_inputs_meet_their_conditions(shape):
    """75 - 95 % of the pairs have a common time, 40 - 60 % a delay > 0, and in every launch at least 25 % of the finite queries have the
    time strictly inside the clamped window: by the pair entry's float64 restatement on the host."""
    m, n = SHAPES[shape]
    for d in (1, 2, 3):
        fleet = _fleet_inputs(n, m, d)
        start = si.starts_of(fleet)
        common, later = si.input_shares(fleet, start)
        assert 0.75 <= common <= 0.95 and 0.40 <= later <= 0.60, (shape, d, common, later)
        for k in (1, 7, 8):
            lo, hi = si.scene_windows(fleet, start, k, 900 + k)
            a, b, lo_p, hi_p, delay, _ = si.gathered(fleet, start, lo, hi)
            value, time, _ = sr.separation_f64(a, b, lo_p, hi_p, delay)
            as_fleet = lambda v: np.asarray(v, dtype=np.float64).reshape(n, m * (m - 1) // 2, k)      # noqa: E731
            inside, finite = si.share_inside(fleet, start, lo, hi, as_fleet(value), as_fleet(time))
            print("%s d = %d k = %d: common %.3f, delay > 0 %.3f, finite %.3f, strictly inside %.3f" % (shape, d, k, common, later, finite, inside))
            assert inside >= 0.25, (shape, d, k, inside)


@pytest.mark.parametrize("d", (2, 3))
def test_the_derivative_tests_inputs_hold_every_class_of_time(d):
    m, n, k = 5, 30, 7
    fleet = _fleet_inputs(n, m, d)
    start = si.starts_of(fleet)
    lo, hi = si.scene_windows(fleet, start, k, 960 + d)
    a, b, lo_p, hi_p, delay, _ = si.gathered(fleet, start, lo, hi)
    _, time, _ = sr.separation_f64(a, b, lo_p, hi_p, delay)
    cls = sr.classes(a, b, lo_p, hi_p, delay, np.asarray(time, dtype=np.float64))[0]
    share = np.bincount(cls.ravel(), minlength=7) / cls.size
    print("d = %d: LO, HI, END of the first, END of the second, START, interior, none: %s" % (d, np.round(share, 3)))
    assert np.all(share > 0), share
