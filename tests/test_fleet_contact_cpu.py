"""The first contact of every pair of a fleet without a GPU (rp_trajectory_fleet_contact, trajectory_fleet_contact, min_time_fleet_contact,
fleet_first_contact): the entry exists, is bound and exported and is in the header's list; it and the torch layer
refuse bad arguments before any device call; fleet_first_contact, which is plain torch, on tensors made by hand -- NaNs, a scene without a
contact, an exact tie --, its gradient one-hot onto the winner, and torch.autograd.gradcheck."""
import ctypes
import os
import re

import pytest

import rocket_path_amd as rp
from rocket_path_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "rp_batch.h")).read()
    lib = capi.load_library()
    assert re.search(r"RP_API\s+int\s+rp_trajectory_fleet_contact\s*\(", header)
    assert "rp_trajectory_fleet_contact" in capi.SIGNATURES and hasattr(lib, "rp_trajectory_fleet_contact")
    text = header[header.index("the first contact of every pair of a fleet"):]
    for word in ("rp_trajectory_contact", "rp_trajectory_fleet_separation", "level_per_pair == 0", "level_per_pair == 1", "n x pairs x k",
                 "bit for bit", "d_delay == NULL", "m - 1 pairs", "SQUARED", "16-byte aligned", "may be NULL", "no batch entry"):
        assert word in text, word
    assert "rp_trajectory_fleet_contact" in header[:header.index("#define RP_ABI_VERSION")]      # in the list of entries
    assert lib.rp_abi_version() == 7      # an entry only: the revision stays
    for name in ("trajectory_fleet_contact", "min_time_fleet_contact", "fleet_first_contact"):
        assert getattr(rp, name).__name__ == name
    assert callable(capi.trajectory_fleet_contact)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.load_library()
    buf = (ctypes.c_double * 8)()                     # host memory: never dereferenced, the checks come first
    good = ctypes.addressof(buf) & ~15
    odd = good + 8
    vp = ctypes.c_void_p
    entry, bad = lib.rp_trajectory_fleet_contact, capi.RP_ERR_INVALID
    g = vp(good)
    for d in (1, 2, 3):
        table = capi.axes_table([good] * (8 * d), d)
        for per_pair in (0, 1):
            for m in (1, 0, 257, 1 << 40):
                assert entry(0, None, 4, m, 4, d, table, g, per_pair, g, g, g, g) == bad and b"m must be 2..256" in lib.rp_last_error(), m
            assert entry(0, None, 0, 3, 4, d, table, g, per_pair, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 0, d, table, g, per_pair, g, g, g, g) == bad and b"positive" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 1 << 31, d, table, g, per_pair, g, g, g, g) == bad and b"2^31" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 4, d, None, g, per_pair, g, g, g, g) == bad and b"d_fleet is null" in lib.rp_last_error()
            assert entry(-1, None, 4, 3, 4, d, table, g, per_pair, g, g, g, g) == bad
            assert entry(0, None, (1 << 63) // 4, 256, 4, d, table, g, per_pair, g, g, g, g) == bad and b"does not fit" in lib.rp_last_error()
            assert entry(0, None, (1 << 60) // 3, 3, 4, d, table, g, per_pair, g, g, g, g) == bad and b"does not fit" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 4, d, table, None, per_pair, g, g, g, g) == bad and b"d_level_sq is null" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 4, d, table, g, per_pair, g, g, None, g) == bad and b"d_time is null" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 4, d, table, g, per_pair, g, g, vp(odd), g) == bad and b"16-byte" in lib.rp_last_error()
            assert entry(0, None, 4, 3, 4, d, table, g, per_pair, g, g, g, vp(odd)) == bad and b"16-byte" in lib.rp_last_error()
        for wrong in (2, -1, 256):
            assert entry(0, None, 4, 3, 4, d, table, g, wrong, g, g, g, g) == bad and b"level_per_pair" in lib.rp_last_error(), wrong
        # a per-pair level moves as 16-byte vectors; a per-scene level and the windows are read as single values: no alignment rule, so an
        # odd one gets as far as the next check, here the misaligned rate
        assert entry(0, None, 4, 3, 4, d, table, vp(odd), 1, g, g, g, g) == bad and b"16-byte" in lib.rp_last_error()
        assert entry(0, None, 4, 3, 4, d, table, vp(odd), 0, vp(odd), vp(odd), g, vp(odd)) == bad and b"16-byte" in lib.rp_last_error()
        for f in range(8 * d):      # the end velocities of any axis may be NULL: those calls fail later, for want of a time
            entries = [good] * (8 * d)
            entries[f] = 0
            assert entry(0, None, 4, 3, 4, d, capi.axes_table(entries, d), g, 0, None, None, None, None) == bad
            assert (b"d_time is null" in lib.rp_last_error()) == (f % 8 in (3, 4)), (d, f)
    big = capi.axes_table([good] * 32, 4)
    for d in (0, 4, -1):      # before the table is looked at
        assert entry(0, None, 4, 3, 4, d, big, g, 0, g, g, g, g) == bad and b"d must be 1, 2 or 3" in lib.rp_last_error(), d
        with pytest.raises(ValueError, match="d must be"):
            capi.trajectory_fleet_contact(0, 0, 4, 3, 4, d, [good] * 8, good, 0, good, good, good, good)
    for m in (1, 257):
        with pytest.raises(ValueError, match="m must be"):
            capi.trajectory_fleet_contact(0, 0, 4, m, 4, 2, [good] * 16, good, 0, good, good, good, good)
    with pytest.raises(ValueError, match="16 entries"):
        capi.trajectory_fleet_contact(0, 0, 4, 3, 4, 2, [good] * 8, good, 0, good, good, good, good)
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact(0, 0, 4, 3, 4, 2, [good] * 16, good, 0, good, good)      # no time
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact(0, 0, 4, 3, 4, 2, [good] * 16, None, 0, good, good, good)      # no level
    with pytest.raises(rp.RpError):
        capi.trajectory_fleet_contact(0, 0, 4, 3, 4, 2, [good] * 16, good, 2, good, good, good)      # neither layout


def test_torch_layer_checks_its_arguments():
    torch = pytest.importorskip("torch")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    x = f64(4, 3, 2)      # n = 4 scenes of m = 3 vehicles (3 pairs) in d = 2 axes
    who, whole = rp.trajectory_fleet_contact, rp.min_time_fleet_contact
    for radius in (f64(4, 5), f64(5), f64(4, 3, 5)):                    # CPU tensors: after every check of shape and type
        with pytest.raises(TypeError, match="ROCm device"):
            who([x] * 6, radius)
        with pytest.raises(TypeError, match="ROCm device"):
            who([x] * 8, None, f64(4, 5), f64(5), level_sq=radius)
        with pytest.raises(TypeError, match="ROCm device"):
            whole([x] * 3, radius, f64(4, 5))
    for call, arg in ((who, [x] * 6), (whole, [x] * 3)):
        with pytest.raises(TypeError, match="either radius or level_sq=, not both"):
            call(arg, f64(4, 5), level_sq=f64(4, 5))
        with pytest.raises(TypeError, match="either radius or level_sq=, not neither"):
            call(arg)
        with pytest.raises(TypeError, match="either radius or level_sq=, not neither"):
            call(arg, None, f64(4, 5), f64(4, 5))
        for wrong in (f64(4, 4, 5), f64(4, 2, 5), f64(3, 5), f64(3, 3, 5), f64(4, 0), f64(0), f64(4, 3, 0), f64(4, 3, 5, 1), f64()):
            with pytest.raises(ValueError, match="radius must have shape"):      # (n, pairs + 1, k) among them
                call(arg, wrong)
            with pytest.raises(ValueError, match="level_sq must have shape"):
                call(arg, level_sq=wrong)
        with pytest.raises(TypeError, match="float64"):
            call(arg, torch.zeros((4, 5)))
        with pytest.raises(TypeError, match="float64"):
            call(arg, level_sq=torch.zeros((4, 3, 5), dtype=torch.float32))
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(arg, 1.0)
        for wrong in (f64(4, 3, 5), f64(3, 5), f64(4, 0), f64(0)):         # a window per scene and query, not per pair
            with pytest.raises(ValueError, match="lo must have shape"):
                call(arg, f64(4, 5), wrong)
            with pytest.raises(ValueError, match="hi must have shape"):
                call(arg, f64(4, 5), None, wrong)
        with pytest.raises(ValueError, match="lo has shape"):
            call(arg, f64(4, 5), f64(4, 5), f64(4, 6))
        for level in (f64(4, 5), f64(5), f64(4, 3, 5)):
            with pytest.raises(ValueError, match="queries per scene"):
                call(arg, level, f64(4, 6))
            with pytest.raises(ValueError, match="queries per scene"):
                call(arg, None, None, f64(6), level_sq=level)
        with pytest.raises(TypeError, match="float64"):
            call(arg, f64(4, 5), torch.zeros((4, 5)))
    with pytest.raises(TypeError, match="list or tuple"):
        who(x, f64(4, 5))
    with pytest.raises(ValueError, match="six"):
        who([x] * 7, f64(4, 5))
    with pytest.raises(TypeError, match="torch.Tensor"):
        who([x] * 5 + [None], f64(4, 5))
    for wrong in (f64(4, 2), f64(4), f64(4, 3, 2, 1)):                  # always three-dimensional: 2-D fleet tensors are refused
        with pytest.raises(ValueError, match=r"\(n, m, d\)"):
            who([wrong] * 6, f64(4, 5))
        with pytest.raises(ValueError, match=r"\(n, m, d\)"):
            whole([wrong] * 3, f64(4, 5))
    for m in (1, 257):
        with pytest.raises(ValueError, match="2..256 vehicles"):
            who([f64(2, m, 2)] * 6, f64(2, 5))
        with pytest.raises(ValueError, match="2..256 vehicles"):
            whole([f64(2, m, 2)] * 3, f64(2, 5))
    for d in (0, 4):
        with pytest.raises(ValueError, match="axes"):
            who([f64(4, 3, d)] * 6, f64(4, 5))
        with pytest.raises(ValueError, match="d in 1..3"):
            whole([f64(4, 3, d)] * 3, f64(4, 5))
    with pytest.raises(ValueError, match="duration1 has shape"):
        who([x] * 5 + [f64(4, 2, 2)], f64(4, 5))
    with pytest.raises(TypeError, match="float64"):
        who([x] * 5 + [x.float()], f64(4, 5))                          # float32
    with pytest.raises(TypeError, match="three tensors"):
        whole([x] * 2, f64(4, 5))
    with pytest.raises(TypeError, match="pair"):
        whole([x] * 3, f64(4, 5), vel=[x], synchronize=False)
    with pytest.raises(ValueError, match="one shape"):
        whole([x, x, f64(4, 3, 3)], f64(4, 5))
    with pytest.raises(ValueError, match="synchronize=True"):           # end velocities need synchronize=False
        whole([x] * 3, f64(4, 5), vel=(x, x))
    with pytest.raises(ValueError, match="synchronize=True"):
        whole([x] * 3, level_sq=f64(4, 3, 5), vel=(None, x))


def test_first_contact_of_hand_made_scenes():
    torch = pytest.importorskip("torch")
    nan = float("nan")
    # three scenes of three pairs and two queries: [scene, pair, query]
    t = torch.tensor([[[3.0, nan], [1.5, 2.0], [nan, 2.0]],          # query 0: pair 1 at 1.5; query 1: pairs 1 and 2 tie at 2.0 -> pair 1
                      [[nan, nan], [nan, nan], [nan, nan]],          # a scene without a contact
                      [[0.0, 7.0], [0.0, nan], [-1.0, 7.0]]],        # query 0: a time may be negative; query 1: pairs 0 and 2 tie -> pair 0
                     dtype=torch.float64, requires_grad=True)
    first, pair = rp.fleet_first_contact(t)
    assert first.shape == pair.shape == (3, 2) and pair.dtype == torch.int64 and first.dtype == torch.float64
    assert pair.tolist() == [[1, 1], [-1, -1], [2, 0]]
    assert first[0].tolist() == [1.5, 2.0] and first[2].tolist() == [-1.0, 7.0] and torch.isnan(first[1]).all()
    assert not pair.requires_grad
    # the gradient of t_first[s, q] goes to exactly the winning (pair, q) entry, the upstream's bits; nothing from a scene without a contact
    g = torch.tensor([[2.0, 3.0], [5.0, 7.0], [11.0, 13.0]], dtype=torch.float64)
    (bar,) = torch.autograd.grad(first, t, grad_outputs=g)
    want = torch.zeros_like(bar)
    want[0, 1, 0], want[0, 1, 1], want[2, 2, 0], want[2, 0, 1] = 2.0, 3.0, 11.0, 13.0
    assert torch.equal(bar, want)
    # an infinite time is no contact either; one pair; float32; any device's tensor, here the CPU's
    first, pair = rp.fleet_first_contact(torch.tensor([[[float("inf")], [4.0]], [[float("-inf")], [nan]]], dtype=torch.float64))
    assert pair.tolist() == [[1], [-1]] and first[0, 0].item() == 4.0 and torch.isnan(first[1, 0])
    first, pair = rp.fleet_first_contact(torch.tensor([[[0.25, nan]]], dtype=torch.float32))
    assert first.dtype == torch.float32 and pair.tolist() == [[0, -1]] and first[0, 0].item() == 0.25 and torch.isnan(first[0, 1])
    for wrong in (torch.zeros((3, 2), dtype=torch.float64), torch.zeros((3, 0, 2), dtype=torch.float64), torch.zeros((3, 2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\(n, pairs, k\)"):
            rp.fleet_first_contact(wrong)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rp.fleet_first_contact([[1.0]])


def test_first_contact_gradcheck():
    torch = pytest.importorskip("torch")
    gen = torch.Generator().manual_seed(27)
    t = torch.rand((3, 6, 4), dtype=torch.float64, generator=gen)      # distinct times: the winner does not change under gradcheck's steps
    t = (t + torch.arange(6, dtype=torch.float64).reshape(1, 6, 1)[:, torch.randperm(6, generator=gen), :] * 2.0).requires_grad_()
    assert torch.autograd.gradcheck(lambda x: rp.fleet_first_contact(x)[0], (t,))
    first, pair = rp.fleet_first_contact(t)
    assert torch.equal(first, t.detach().amin(dim=1)) and torch.equal(pair, t.detach().argmin(dim=1))
