"""The closest approach of every pair of a fleet without a GPU (rp_trajectory_fleet_separation, fleet_pairs, trajectory_fleet_separation,
min_time_fleet_separation): the kernel's pair decode (csrc/fleet_index.h) compiled for the host with the address and
undefined-behaviour sanitizers into a stand-alone program, for every fleet size against itertools.combinations; fleet_pairs and the
derivative routing's slot table against the same order; the entry exists and refuses bad arguments before any device call, and so does
the torch layer."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rocket_path_amd as rp
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = r"""
#include <cstdio>
#include <vector>
#include "fleet_index.h"
int main()
{
    static_assert(rp::kFleetMost == 256, "the largest fleet");
    for (unsigned m = 2; m <= rp::kFleetMost; ++m) {
        const unsigned pairs = rp::fleet_pair_count(m);
        std::vector<unsigned short> out(2 * (size_t)pairs);
        for (unsigned r = 0; r < pairs; ++r) {
            unsigned i = ~0u, j = ~0u;
            rp::fleet_pair(r, m, i, j);
            if (!(i < j && j < m)) return 1;
            out[2 * r] = (unsigned short)i;
            out[2 * r + 1] = (unsigned short)j;
        }
        if (fwrite(out.data(), sizeof(unsigned short), out.size(), stdout) != out.size()) return 2;
    }
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pair_decode_on_the_host_is_combinations_order_for_every_fleet_size(tmp_path):
    src, exe = tmp_path / "decode.cpp", tmp_path / "decode"
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "rocket_path_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    got = np.frombuffer(r.stdout, dtype=np.uint16)
    at = 0
    for m in range(2, 257):
        count = m * (m - 1)
        want = np.fromiter(itertools.chain.from_iterable(itertools.combinations(range(m), 2)), dtype=np.uint16, count=count)
        assert np.array_equal(got[at:at + count], want), m
        at += count
    assert at == len(got)


def test_fleet_pairs_and_the_slot_table():
    torch = pytest.importorskip("torch")
    from rocket_path_amd import autograd
    for m in (2, 3, 4, 5, 17, 64, 256):
        pairs = rp.fleet_pairs(m)
        assert pairs.dtype == torch.int64 and pairs.shape == (m * (m - 1) // 2, 2)
        assert [tuple(p) for p in pairs.tolist()] == list(itertools.combinations(range(m), 2)), m
        assert torch.equal(pairs, torch.triu_indices(m, m, 1).t())
        pair, sign, partner = (t.numpy() for t in autograd.fleet_slots(m))
        assert pair.shape == sign.shape == partner.shape == (m, m - 1)
        # the pairs' inverse: every pair exactly once in each of its two vehicles' rows, +1 in its first vehicle's and -1 in its second's
        assert np.all(np.diff(partner, axis=1) > 0) and all(v not in partner[v] for v in range(m)), m
        p = pairs.numpy()
        rows = np.repeat(np.arange(m)[:, None], m - 1, axis=1)
        assert np.array_equal(p[pair, 0], np.minimum(rows, partner)) and np.array_equal(p[pair, 1], np.maximum(rows, partner)), m
        assert np.array_equal(sign, np.where(rows < partner, 1.0, -1.0)), m
        for want_sign, column in ((1.0, 0), (-1.0, 1)):
            where = sign == want_sign
            assert np.array_equal(np.sort(pair[where]), np.arange(len(p))), m      # each pair once with each sign ...
            assert np.array_equal(rows[where][np.argsort(pair[where])], p[:, column]), m      # ... in that vehicle's row
    for bad in (1, 0, 257, -3):
        with pytest.raises(ValueError, match="2..256"):
            rp.fleet_pairs(bad)
    with pytest.raises(TypeError):
        rp.fleet_pairs(2.0)


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+rp_trajectory_fleet_separation\s*\(", header)
    assert "rp_trajectory_fleet_separation" in capi.SIGNATURES and hasattr(lib, "rp_trajectory_fleet_separation")
    text = header[header.index("the closest approach of every pair of a fleet"):]
    for word in ("2 <= m <= 256", "axis-major", "s m + v", "lexicographic", "n x pairs x k", "bit for bit", "d_delay == NULL", "m - 1 pairs",
                 "either may be NULL", "no batch entry", "No pair-expanded array"):
        assert word in text, word
    assert "rp_trajectory_fleet_separation" in header[:header.index("#define RP_ABI_VERSION")]      # in the list of entries
    assert lib.rp_abi_version() == 7      # an entry only: the revision stays
    for name in ("fleet_pairs", "trajectory_fleet_separation", "min_time_fleet_separation"):
        assert getattr(rp, name).__name__ == name
    assert callable(capi.trajectory_fleet_separation)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    fleet, bad = lib.rp_trajectory_fleet_separation, capi.RP_ERR_INVALID
    g = vp(good)
    for d in (1, 2, 3):
        table = capi.axes_table([good] * (8 * d), d)
        for m in (1, 0, 257, 1 << 40):
            assert fleet(0, None, 4, m, 4, d, table, g, g, g, g) == bad and b"m must be 2..256" in lib.rp_last_error(), m
        assert fleet(0, None, 0, 3, 4, d, table, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
        assert fleet(0, None, 4, 3, 0, d, table, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
        assert fleet(0, None, 4, 3, 1 << 31, d, table, g, g, g, g) == bad and b"2^31" in lib.rp_last_error()
        assert fleet(0, None, 4, 3, 4, d, None, g, g, g, g) == bad and b"d_fleet is null" in lib.rp_last_error()
        assert fleet(-1, None, 4, 3, 4, d, table, g, g, g, g) == bad
        assert fleet(0, None, (1 << 63) // 4, 256, 4, d, table, g, g, g, g) == bad and b"does not fit" in lib.rp_last_error()
        for f in range(8 * d):      # the end velocities of any axis may be NULL: those calls fail later, for want of an output
            entries = [good] * (8 * d)
            entries[f] = 0
            assert fleet(0, None, 4, 3, 4, d, capi.axes_table(entries, d), None, None, None, None) == bad
            assert (b"no output" in lib.rp_last_error()) == (f % 8 in (3, 4)), (d, f)
        # both outputs NULL; either alone is allowed and gets as far as the alignment; the windows are read as single values
        assert fleet(0, None, 4, 3, 4, d, table, g, g, None, None) == bad and b"no output" in lib.rp_last_error()
        assert fleet(0, None, 4, 3, 4, d, table, g, g, vp(odd), None) == bad and b"16-byte" in lib.rp_last_error()
        assert fleet(0, None, 4, 3, 4, d, table, g, g, None, vp(odd)) == bad and b"16-byte" in lib.rp_last_error()
    big = capi.axes_table([good] * 32, 4)
    for d in (0, 4, -1):      # before the table is looked at
        assert fleet(0, None, 4, 3, 4, d, big, g, g, g, g) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_separation(0, 0, 4, 3, 4, d, [good] * 8, good, good, good, good)
    for m in (1, 257):
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_separation(0, 0, 4, m, 4, 2, [good] * 16, good, good, good, good)
    with pytest.raises(ValueError, match="16 entries"):
        capi.trajectory_fleet_separation(0, 0, 4, 3, 4, 2, [good] * 8, good, good, good, good)
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_separation(0, 0, 4, 3, 4, 2, [good] * 16, good, good)      # no output


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    x = f64(4, 3, 2)
    who = rp.trajectory_fleet_separation
    with pytest.raises(TypeError, match="ROCm device"):
        who([x] * 6)                                                    # CPU tensors: after every check of shape and type
    with pytest.raises(TypeError, match="ROCm device"):
        who([x] * 8, f64(4, 5), f64(5))
    with pytest.raises(TypeError, match="list or tuple"):
        who(x)
    with pytest.raises(ValueError, match="six"):
        who([x] * 7)
    with pytest.raises(TypeError, match="torch.Tensor"):
        who([[0.0]] + [x] * 5)
    with pytest.raises(TypeError, match="torch.Tensor"):
        who([x] * 5 + [None])
    for wrong in (f64(4, 2), f64(4), f64(4, 3, 2, 1)):                  # always three-dimensional
        with pytest.raises(ValueError, match=r"\(n, m, d\)"):
            who([wrong] * 6)
    for m in (1, 257):
        with pytest.raises(ValueError, match="2..256 vehicles"):
            who([f64(2, m, 2)] * 6)
        with pytest.raises(ValueError, match="2..256 vehicles"):
            rp.min_time_fleet_separation([f64(2, m, 2)] * 3)
    for d in (0, 4):
        with pytest.raises(ValueError, match="axes"):
            who([f64(4, 3, d)] * 6)
        with pytest.raises(ValueError, match="d in 1..3"):
            rp.min_time_fleet_separation([f64(4, 3, d)] * 3)
    with pytest.raises(ValueError, match="duration1 has shape"):
        who([x] * 5 + [f64(4, 2, 2)])
    with pytest.raises(ValueError, match="vel2 has shape"):
        who([x] * 7 + [f64(3, 3, 2)])
    with pytest.raises(TypeError, match="float64"):
        who([x] * 5 + [x.float()])
    for wrong in (f64(4, 3, 5), f64(3, 5), f64(4, 0), f64(0)):         # a window per scene and query, not per pair
        with pytest.raises(ValueError, match="lo must have shape"):
            who([x] * 6, wrong)
        with pytest.raises(ValueError, match="hi must have shape"):
            rp.min_time_fleet_separation([x] * 3, None, wrong)
    with pytest.raises(TypeError, match="float64"):
        who([x] * 6, torch.zeros((4, 5)))
    with pytest.raises(TypeError, match="float64"):
        who([x] * 6, None, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="lo has shape"):
        who([x] * 6, f64(4, 5), f64(4, 6))
    with pytest.raises(TypeError, match="three tensors"):
        rp.min_time_fleet_separation([x] * 2)
    with pytest.raises(TypeError, match="pair"):
        rp.min_time_fleet_separation([x] * 3, vel=[x], synchronize=False)
    with pytest.raises(ValueError, match="one shape"):
        rp.min_time_fleet_separation([x, x, f64(4, 3, 3)])
    with pytest.raises(ValueError, match="synchronize=True"):           # before anything else
        rp.min_time_fleet_separation([x] * 3, vel=(x, x))
    with pytest.raises(ValueError, match="synchronize=True"):
        rp.min_time_fleet_separation([x] * 2, vel=(None, x))
    with pytest.raises(TypeError, match="ROCm device"):
        rp.min_time_fleet_separation([x] * 3, f64(4, 5))
