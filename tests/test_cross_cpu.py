"""One fleet's vehicles against another's without a GPU (rp_trajectory_cross_separation, rp_trajectory_cross_contact; cross_pairs,
static_fleet, trajectory_cross_separation, trajectory_cross_contact, min_time_cross_separation, min_time_cross_contact; DESIGN.md section
34): the entries exist, are bound and exported and the revision stays; they, their ctypes mirrors and the torch layer refuse bad arguments
before any device call; the kernel's pair decode (csrc/fleet_index.h) compiled for the host with the address and undefined-behaviour
sanitizers into a stand-alone program against divmod; cross_pairs against numpy.indices; static_fleet through the evaluator's longdouble
reference."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rocket_path_amd as rp
import trajectory_ref as tr
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rp_trajectory_cross_separation", "rp_trajectory_cross_contact")
CALLS = ("cross_pairs", "static_fleet", "trajectory_cross_separation", "trajectory_cross_contact", "min_time_cross_separation",
         "min_time_cross_contact")


def test_entries_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"RP_API\s+int\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
        assert name in header[:header.index("#define RP_ABI_VERSION")], name      # in the list of entries
    text = header[header.index("the vehicles of one fleet against the vehicles of another"):]
    text = text[:text.index("rp_trajectory_cross_contact(")]
    for word in ("1 <= m_a, m_b <= 32768", "s m_a + v", "s m_b + v", "(r / m_b, r % m_b)", "n x m_a x m_b x k", "bit for bit", "d_delay == NULL",
                 "rp_trajectory_separation", "rp_trajectory_contact", "exactly its row", "exactly its column", "level_per_pair == 0", "16-byte aligned",
                 "[3] and [4]", "either may be NULL but not both", "may be NULL", "no batch entry", "before any device call"):
        assert word in text, word
    assert lib.rp_abi_version() == 7 and capi.ABI_VERSION == 7      # entries only: the revision stays
    for name in CALLS:
        assert getattr(rp, name).__name__ == name
    assert callable(capi.trajectory_cross_separation) and callable(capi.trajectory_cross_contact)


def test_the_c_entries_refuse_bad_arguments_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    vp = ctypes.c_void_p
    g, odd, bad = vp(good), vp(good + 8), capi.RP_ERR_INVALID
    sep, con = lib.rp_trajectory_cross_separation, lib.rp_trajectory_cross_contact
    err = lib.rp_last_error

    def refused(what, *, n=4, m_a=3, m_b=5, k=4, d=2, a="table", b="table", level=g, per_pair=0, lo=g, hi=g, out=(g, g), device=0, only=None):
        """both entries with these arguments: RP_ERR_INVALID, with `what` in the message"""
        table = capi.axes_table([good] * (8 * max(1, min(d, 3))), max(1, min(d, 3)))
        ta, tb = (table if t == "table" else t for t in (a, b))
        for entry in (sep, con):
            if only is not None and entry is not only:
                continue
            middle = (level, per_pair) if entry is con else ()
            assert entry(device, None, n, m_a, m_b, k, d, ta, tb, *middle, lo, hi, *out) == bad, (what, entry.__name__)
            assert what in err(), (what, entry.__name__, err())

    for m in (0, 32769, 1 << 40):
        refused(b"m_a and m_b must be 1..32768", m_a=m)
        refused(b"m_a and m_b must be 1..32768", m_b=m)
    for d in (0, 4, -1):
        refused(b"d must be 1, 2 or 3", d=d)
    refused(b"d_fleet_a is null", a=None)
    refused(b"d_fleet_b is null", b=None)
    refused(b"device", device=-1)
    refused(b"no output asked for", out=(None, None), only=sep)
    refused(b"d_level_sq is null", level=None, only=con)
    refused(b"d_time is null", out=(None, g), only=con)
    for wrong in (2, -1, 256):
        refused(b"level_per_pair", per_pair=wrong, only=con)
    refused(b"16-byte", out=(odd, g))
    refused(b"16-byte", out=(g, odd))
    refused(b"16-byte", level=odd, per_pair=1, only=con)
    refused(b"positive", n=0)
    refused(b"positive", k=0)
    refused(b"2^31", k=1 << 31)
    refused(b"does not fit", n=(1 << 63) // 4, m_a=32768, m_b=32768)
    refused(b"does not fit", n=(1 << 60) // 15)
    # a per-scene level and the windows are read as single values: no alignment rule, so odd ones get as far as the next check, here the
    # misaligned second output
    refused(b"16-byte", level=odd, per_pair=0, lo=odd, hi=odd, out=(g, odd))
    # the largest fleets pass the size check (the next one, here the outputs, refuses)
    refused(b"no output asked for", m_a=32768, m_b=32768, out=(None, None), only=sep)
    refused(b"d_time is null", m_a=1, m_b=1, out=(None, g), only=con)
    for d in (1, 2, 3):
        for side in range(2):      # the end velocities of any axis of either table may be NULL: those calls fail later, for want of an output
            for f in range(8 * d):
                entries = [good] * (8 * d)
                entries[f] = 0
                tables = [capi.axes_table([good] * (8 * d), d), capi.axes_table([good] * (8 * d), d)]
                tables[side] = capi.axes_table(entries, d)
                assert sep(0, None, 4, 3, 5, 4, d, tables[0], tables[1], None, None, None, None) == bad
                assert (b"no output asked for" in err()) == (f % 8 in (3, 4)), (d, side, f, err())
                assert con(0, None, 4, 3, 5, 4, d, tables[0], tables[1], g, 0, None, None, None, None) == bad
                assert (b"d_time is null" in err()) == (f % 8 in (3, 4)), (d, side, f, err())


def test_the_ctypes_mirrors_refuse_bad_arguments():
    buf = (ctypes.c_double * 8)()
    good = ctypes.addressof(buf) & ~15
    sep, con = capi.trajectory_cross_separation, capi.trajectory_cross_contact
    for d in (0, 4, -1):
        with pytest.raises(ValueError, match="d must be"):
            sep(0, 0, 4, 3, 5, 4, d, [good] * 8, [good] * 8, good, good, good, good)
        with pytest.raises(ValueError, match="d must be"):
            con(0, 0, 4, 3, 5, 4, d, [good] * 8, [good] * 8, good, 0, good, good, good, good)
    for m_a, m_b in ((0, 5), (3, 0), (32769, 5), (3, 32769)):
        with pytest.raises(ValueError, match="m_a and m_b must be"):
            sep(0, 0, 4, m_a, m_b, 4, 2, [good] * 16, [good] * 16, good, good, good, good)
        with pytest.raises(ValueError, match="m_a and m_b must be"):
            con(0, 0, 4, m_a, m_b, 4, 2, [good] * 16, [good] * 16, good, 0, good, good, good, good)
    with pytest.raises(ValueError, match="16 entries"):
        sep(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 8, good, good, good, good)
    with pytest.raises(ValueError, match="16 entries"):
        con(0, 0, 4, 3, 5, 4, 2, [good] * 8, [good] * 16, good, 0, good, good, good, good)
    with pytest.raises(rp.RpError):
        sep(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 16, good, good)      # no output
    with pytest.raises(rp.RpError):
        con(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 16, good, 0, good, good)      # no time
    with pytest.raises(rp.RpError):
        con(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 16, None, 0, good, good, good)      # no level
    with pytest.raises(rp.RpError):
        con(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 16, good, 2, good, good, good)      # neither layout
    with pytest.raises(rp.RpError):
        con(0, 0, 4, 3, 5, 4, 2, [good] * 16, [good] * 16, good + 8, 1, good, good, good)      # a misaligned per-pair level
    with pytest.raises(rp.RpError):
        sep(0, 0, 0, 3, 5, 4, 2, [good] * 16, [good] * 16, good, good, good, good)      # n = 0


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    a, b = f64(4, 3, 2), f64(4, 5, 2)      # n = 4 scenes, m_a = 3 against m_b = 5 (15 pairs) in d = 2 axes
    sep, con, whole_sep, whole_con = rp.trajectory_cross_separation, rp.trajectory_cross_contact, rp.min_time_cross_separation, rp.min_time_cross_contact
    # CPU tensors: after every check of shape and type, a fleet of one on either side included
    for fa, fb in (([a] * 6, [b] * 6), ([a] * 8, [b] * 6), ([f64(4, 1, 2)] * 6, [b] * 6), ([a] * 6, [f64(4, 1, 2)] * 6)):
        pairs = fa[0].shape[1] * fb[0].shape[1]
        with pytest.raises(TypeError, match="ROCm device"):
            sep(fa, fb, f64(4, 6), f64(6))
        for radius in (f64(4, 6), f64(6), f64(4, pairs, 6), f64(4, fa[0].shape[1], fb[0].shape[1], 6)):
            with pytest.raises(TypeError, match="ROCm device"):
                con(fa, fb, radius)
            with pytest.raises(TypeError, match="ROCm device"):
                con(fa, fb, None, f64(4, 6), level_sq=radius)
    with pytest.raises(TypeError, match="ROCm device"):
        whole_sep([a] * 3, [b] * 3, f64(4, 6))
    with pytest.raises(TypeError, match="ROCm device"):
        whole_con([a] * 3, [b] * 3, f64(4, 3, 5, 6))
    for call, fa, fb in ((con, [a] * 6, [b] * 6), (whole_con, [a] * 3, [b] * 3)):
        with pytest.raises(TypeError, match="either radius or level_sq=, not both"):
            call(fa, fb, f64(4, 6), level_sq=f64(4, 6))
        with pytest.raises(TypeError, match="either radius or level_sq=, not neither"):
            call(fa, fb)
        with pytest.raises(TypeError, match="either radius or level_sq=, not neither"):
            call(fa, fb, None, f64(4, 6), f64(4, 6))
        for wrong in (f64(4, 5, 3, 6), f64(4, 3, 4, 6), f64(3, 3, 5, 6), f64(4, 3, 5, 0), f64(4, 15, 1, 6)):      # m_a m_b is wrong, or n, or k
            with pytest.raises(ValueError, match="four-dimensional radius must have shape"):
                call(fa, fb, wrong)
            with pytest.raises(ValueError, match="four-dimensional level_sq must have shape"):
                call(fa, fb, level_sq=wrong)
        for wrong in (f64(4, 14, 6), f64(4, 16, 6), f64(3, 6), f64(4, 0), f64(0), f64(4, 15, 0), f64(4, 3, 5, 6, 1), f64()):
            with pytest.raises(ValueError, match="radius must have shape"):
                call(fa, fb, wrong)
            with pytest.raises(ValueError, match="level_sq must have shape"):
                call(fa, fb, level_sq=wrong)
        with pytest.raises(TypeError, match="float64"):
            call(fa, fb, torch.zeros((4, 6)))                               # float32
        with pytest.raises(TypeError, match="float64"):
            call(fa, fb, level_sq=torch.zeros((4, 3, 5, 6), dtype=torch.float32))
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(fa, fb, 1.0)
        for level in (f64(4, 6), f64(6), f64(4, 15, 6), f64(4, 3, 5, 6)):
            with pytest.raises(ValueError, match="queries per scene"):
                call(fa, fb, level, f64(4, 7))
            with pytest.raises(ValueError, match="queries per scene"):
                call(fa, fb, None, None, f64(7), level_sq=level)
    for call, fa, fb in ((sep, [a] * 6, [b] * 6), (whole_sep, [a] * 3, [b] * 3)):
        for wrong in (f64(4, 15, 6), f64(3, 6), f64(4, 0), f64(0)):         # a window per scene and query, not per pair
            with pytest.raises(ValueError, match="lo must have shape"):
                call(fa, fb, wrong)
            with pytest.raises(ValueError, match="hi must have shape"):
                call(fa, fb, None, wrong)
        with pytest.raises(ValueError, match="lo has shape"):
            call(fa, fb, f64(4, 6), f64(4, 7))
        with pytest.raises(TypeError, match="float64"):
            call(fa, fb, torch.zeros((4, 6)))
    # the fleets themselves
    for call in (sep, lambda x, y: con(x, y, f64(4, 6))):
        with pytest.raises(TypeError, match="list or tuple"):
            call(a, [b] * 6)
        with pytest.raises(TypeError, match="list or tuple"):
            call([a] * 6, b)
        with pytest.raises(ValueError, match="six"):
            call([a] * 7, [b] * 6)
        with pytest.raises(TypeError, match="torch.Tensor"):
            call([a] * 6, [b] * 5 + [None])
        for wrong in (f64(4, 2), f64(4), f64(4, 3, 2, 1)):                  # always three-dimensional: 2-D fleet tensors are refused
            with pytest.raises(ValueError, match=r"fleet_a: pos0 must have shape \(n, m, d\)"):
                call([wrong] * 6, [b] * 6)
            with pytest.raises(ValueError, match=r"fleet_b: pos0 must have shape \(n, m, d\)"):
                call([a] * 6, [wrong] * 6)
        with pytest.raises(ValueError, match="share their scenes and their axes"):
            call([a] * 6, [f64(5, 5, 2)] * 6)                              # different n
        with pytest.raises(ValueError, match="share their scenes and their axes"):
            call([a] * 6, [f64(4, 5, 3)] * 6)                              # different d
        for m in (0, 32769):
            with pytest.raises(ValueError, match="1..32768 vehicles"):
                call([f64(4, m, 1)] * 6, [b] * 6)
            with pytest.raises(ValueError, match="1..32768 vehicles"):
                call([a] * 6, [f64(4, m, 2)] * 6)
        for d in (0, 4):
            with pytest.raises(ValueError, match="axes"):
                call([f64(4, 3, d)] * 6, [f64(4, 5, d)] * 6)
        with pytest.raises(ValueError, match="fleet_b: duration1 has shape"):
            call([a] * 6, [b] * 5 + [f64(4, 4, 2)])
        with pytest.raises(TypeError, match="float64"):
            call([a] * 5 + [a.float()], [b] * 6)                           # float32
        with pytest.raises(TypeError, match="float64"):
            call([a] * 6, [b] * 5 + [b.float()])
    for whole in (whole_sep, lambda x, y, **kw: whole_con(x, y, f64(4, 6), **kw)):
        with pytest.raises(TypeError, match="three tensors"):
            whole([a] * 2, [b] * 3)
        with pytest.raises(ValueError, match="one shape"):
            whole([a] * 3, [b, b, f64(4, 5, 3)])
        for wrong in (f64(4, 2), f64(4)):
            with pytest.raises(ValueError, match=r"\(n, m, d\)"):
                whole([a] * 3, [wrong] * 3)
        with pytest.raises(ValueError, match="share their scenes and their axes"):
            whole([a] * 3, [f64(5, 5, 2)] * 3)
        with pytest.raises(ValueError, match="1..32768 vehicles"):
            whole([a] * 3, [f64(4, 0, 2)] * 3)
        with pytest.raises(ValueError, match="synchronize=True"):           # end velocities need synchronize=False
            whole([a] * 3, [b] * 3, vel_b=(b, b))
        with pytest.raises(TypeError, match="pair"):
            whole([a] * 3, [b] * 3, vel_a=[a], synchronize=False)
    # the fleet functions keep their own size rule
    with pytest.raises(ValueError, match="2..256 vehicles"):
        rp.trajectory_fleet_separation([f64(4, 1, 2)] * 6)
    with pytest.raises(ValueError, match="2..256 vehicles"):
        rp.min_time_fleet_contact([f64(4, 257, 2)] * 3, f64(4, 6))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_pair_decode_on_the_host_under_the_sanitizers(tmp_path):
    exe, out = tmp_path / "cross_index_check", tmp_path / "pairs"
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rocket_path_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "cross_index_check.cpp")])

    def decoded(m_a, m_b, first, count):
        r = subprocess.run([str(exe), str(m_a), str(m_b), str(first), str(count), str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (m_a, m_b, first, count, r.returncode, r.stderr[-2000:])
        words = np.fromfile(str(out), dtype=np.uint32)
        assert words[0] == m_a * m_b and len(words) == 1 + 2 * count
        return words[1:].reshape(count, 2)

    for m_a, m_b in ((1, 1), (1, 7), (7, 1), (3, 5), (256, 300)):      # every r
        pairs = m_a * m_b
        assert decoded(m_a, m_b, 0, pairs).tolist() == [list(divmod(r, m_b)) for r in range(pairs)], (m_a, m_b)
    m = 32768      # at the ends: the first pairs, those around the first row's end, and the last, 2^30 - 1 = (32767, 32767)
    for first, count in ((0, 300), (m - 150, 300), (m * m - 300, 300)):
        assert decoded(m, m, first, count).tolist() == [list(divmod(r, m)) for r in range(first, first + count)], first
    assert decoded(m, m, m * m - 1, 1).tolist() == [[m - 1, m - 1]]
    r = subprocess.run([str(exe), "3", "5", "10", "6", str(out)], capture_output=True, text=True)      # past the last pair: refused
    assert r.returncode == 3 and not r.stderr


def test_cross_pairs_against_numpy_indices():
    torch = pytest.importorskip("torch")
    for m_a, m_b in ((1, 1), (1, 7), (7, 1), (3, 5), (16, 200), (256, 300)):
        got = rp.cross_pairs(m_a, m_b)
        assert got.dtype == torch.int64 and got.shape == (2, m_a * m_b) and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), np.indices((m_a, m_b)).reshape(2, -1)), (m_a, m_b)
    i, j = rp.cross_pairs(3, 5)
    assert torch.equal(i * 5 + j, torch.arange(15))      # pair (i, j) is at i m_b + j
    for wrong in ((0, 5), (3, 0), (32769, 1), (1, 32769)):
        with pytest.raises(ValueError, match="1..32768 vehicles"):
            rp.cross_pairs(*wrong)
    for wrong in ((3.0, 5), (3, True)):
        with pytest.raises(TypeError, match="ints"):
            rp.cross_pairs(*wrong)


def test_static_fleet_stands_still():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(34)
    points = rng.uniform(-50, 50, (3, 4, 2))
    for duration in (1.0, 7.5):
        fleet = rp.static_fleet(torch.tensor(points), duration)
        assert len(fleet) == 6 and all(t.shape == (3, 4, 2) and t.dtype == torch.float64 for t in fleet)
        pos0, pos1, pos2, vel1, duration0, duration1 = (t.numpy() for t in fleet)
        assert np.array_equal(pos0, points) and np.array_equal(pos1, points) and np.array_equal(pos2, points)
        assert not vel1.any() and np.all(duration0 == duration / 2) and np.all(duration1 == duration / 2)
        assert duration0 is not duration1 and fleet[4].data_ptr() != fleet[5].data_ptr()
        # through the evaluator's reference, in the table's order with zero end velocities: the position constant, the velocity 0 --
        # before the start, at it, inside each segment, at the knot, at the end and past it
        flat = lambda x: x.reshape(-1)      # noqa: E731
        zero = np.zeros(points.size)
        spline = [flat(pos0), flat(pos1), flat(pos2), zero, zero, flat(vel1), flat(duration0), flat(duration1)]
        tau = np.tile(np.array([-0.25, 0.0, 0.2, 0.5, 0.7, 1.0, 1.25]) * duration, (points.size, 1))
        pos, vel, acc = tr.forward_ld(spline, tau)
        assert np.all(pos == flat(points)[:, None]) and not np.any(vel) and not np.any(acc)
    # differentiable in the points by composition: each of pos0, pos1, pos2 is the points
    leaf = torch.tensor(points, requires_grad=True)
    fleet = rp.static_fleet(leaf)
    (g,) = torch.autograd.grad(sum((w + 1.0) * fleet[w].sum() for w in range(3)), leaf)
    assert torch.equal(g, torch.full_like(g, 6.0)) and not any(t.requires_grad for t in fleet[3:])
    with pytest.raises(ValueError, match=r"\(n, m, d\)"):
        rp.static_fleet(torch.zeros((4, 2), dtype=torch.float64))
    with pytest.raises(TypeError, match="float64"):
        rp.static_fleet(torch.zeros((3, 4, 2)))
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.static_fleet(points)
    for duration in (0.0, -1.0, float("inf"), float("nan")):      # the durations must be positive and finite, or the NaN rule bites
        with pytest.raises(ValueError, match="finite and positive"):
            rp.static_fleet(torch.zeros((3, 4, 2), dtype=torch.float64), duration)
