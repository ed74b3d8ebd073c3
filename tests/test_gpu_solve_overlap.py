"""Back-to-back fused solves of batches that share a stream overlap on an auxiliary stream (rp_solve_overlap_set, include/rp_batch.h):
nothing a caller can read changes.  Every case issues one call sequence twice -- with the overlap off (mode 0: every call on the batch's
stream) and with every eligible solve overlapped (mode 2) -- and compares states, iteration counts and status words bit for bit; the
counters of rp_solve_overlap_stats say whether the auxiliary stream was, or was not, used.  F3 in double precision; n = 1,000 (a ragged
last chunk) and n = 65,536 (a solve of some 25 us: long enough for a missing dependency to show).  Absolute correctness is the oracle
tests' business."""
import ctypes

import numpy as np
import pytest

import rocket_path_amd as rp
from hip_util import DeviceBuffer, _hip

pytestmark = pytest.mark.gpu

SIZES = [1000, 65536]
_problems = {}


def problems(seed, n):
    if (seed, n) not in _problems:
        _problems[seed, n] = rp.problems.generate(seed, 0, n, rp.problems.DIST_MONOTONE)
    return _problems[seed, n]


@pytest.fixture(autouse=True)
def default_mode_afterwards():
    yield
    rp.solve_overlap(1)


def read(b):
    it, st = b.get_iters()
    return [b.get_state(), it, st]


def run(mode, sequence):
    """The sequence under `mode`: what it returns (a list of arrays) and by how much each counter rose."""
    rp.solve_overlap(mode)
    before = rp.solve_overlap_stats()
    out = sequence()
    after = rp.solve_overlap_stats()
    return out, {k: after[k] - before[k] for k in after}


def both_modes(sequence):
    """Run under mode 0 and mode 2; the results must be equal bit for bit, and mode 0 must count nothing.  Returns mode 2's counts."""
    ref, idle = run(0, sequence)
    got, counts = run(2, sequence)
    assert idle == {"aux": 0, "kept": 0, "joins": 0, "excluded": 0}
    assert len(ref) == len(got) and len(ref) > 0
    for i, (r, g) in enumerate(zip(ref, got)):
        assert r.dtype == g.dtype and r.shape == g.shape and r.tobytes() == g.tobytes(), "array %d differs between mode 0 and mode 2" % i
    return counts, got


def family(n, seeds, materialised=()):
    """One batch per seed on ONE stream (the first owns it), its problems set; those listed in `materialised` with the start written out."""
    lead = rp.Batch(n)
    bs = [lead] + [rp.Batch(n, stream=lead.stream()) for _ in seeds[1:]]
    for j, (b, seed) in enumerate(zip(bs, seeds)):
        b.set_problems(*problems(seed, n))
        if j in materialised:
            b.restart()
    return bs


def close(bs):
    for b in bs[1:]:
        b.close()
    bs[0].close()


@pytest.mark.parametrize("n", SIZES)
def test_eight_batches_back_to_back_on_one_stream(n):
    def sequence():
        bs = family(n, list(range(101, 109)), materialised=(1, 2, 5))      # the START form and the plain form of the kernel, mixed
        try:
            for b in bs:
                b.solve(1e-8, 200, 0)
            return [a for b in bs for a in read(b)]
        finally:
            close(bs)
    counts, got = both_modes(sequence)
    assert counts["aux"] >= 3 and counts["excluded"] == 0
    assert all(np.all(st & rp.ST_CONVERGED) for st in got[2::3])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("chain", ["restart", "solve_twice", "set_problems_device", "step", "reduce_device", "events"])
def test_dependency_chains_on_one_batch_among_others(n, chain):
    def sequence():
        a, b, c = bs = family(n, [11, 12, 13], materialised=(2,))
        extra = []
        try:
            if chain == "restart":
                a.solve(); b.solve(); b.restart(); b.solve(); c.solve()
            elif chain == "solve_twice":
                a.solve(); b.solve(); b.solve(); c.solve()      # the second finds everything converged
            elif chain == "set_problems_device":
                with DeviceBuffer(3 * 8 * n) as pos:
                    pos.write(np.stack(problems(14, n)))
                    a.solve()
                    b.set_problems_device(pos.ptr, pos.ptr + 8 * n, pos.ptr + 16 * n)
                    b.solve(); a.solve(); c.solve()
                    b.sync()      # the positions have been read
            elif chain == "step":
                a.solve(); b.solve(); b.step(3); b.solve(); c.solve()
            elif chain == "reduce_device":
                with DeviceBuffer(32) as out4:
                    a.solve(); b.solve(); c.solve(); a.solve(); b.solve()
                    b.reduce_device(out4.ptr)
                    b.sync()
                    extra.append(out4.read(np.float64))
            else:
                a.event_record(0)
                a.solve(); b.solve(); c.solve(); b.solve()
                a.event_record(1)
                a.sync()
                assert a.event_elapsed_ms(0, 1) > 0.0
            return extra + [x for y in bs for x in read(y)]
        finally:
            close(bs)
    counts, _ = both_modes(sequence)
    assert counts["aux"] >= 1 and counts["joins"] >= 1 and counts["excluded"] == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("why", ["bound_buffer", "field_ptr", "handoff_rounds", "steps_per_launch"])
def test_excluded_solves_stay_on_the_callers_stream(n, why):
    hip = _hip()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    rec = np.dtype(rp.capi.SOLUTION_FIELDS)

    def sequence():
        a, b = bs = family(n, [21, 22], materialised=(0, 1))
        extra = []
        try:
            if why == "bound_buffer":
                with DeviceBuffer(32 * n, fill=0xff) as ra, DeviceBuffer(32 * n, fill=0xff) as rb, DeviceBuffer(64 * n, fill=0xff) as copy:
                    a.bind_solution(ra.ptr)
                    b.bind_solution(rb.ptr)
                    a.solve(); b.solve()
                    # foreign work on the stream handle: it must find both sets of records written
                    stream = a.stream()
                    assert hip.hipMemcpyAsync(copy.ptr, ra.ptr, 32 * n, 3, stream) == 0
                    assert hip.hipMemcpyAsync(copy.ptr + 32 * n, rb.ptr, 32 * n, 3, stream) == 0
                    assert hip.hipStreamSynchronize(stream) == 0
                    records = copy.read(rec)
                    assert np.all(records["status"] & rp.ST_CONVERGED) and np.all(records["iters"] > 0)
                    extra.append(records.view(np.uint8))
            elif why == "field_ptr":
                a.field_ptr(0)
                b.field_ptr(0)
                a.solve(); b.solve()
            elif why == "handoff_rounds":
                a.set_params(handoff_rounds=3)
                b.set_params(handoff_rounds=3)
                a.solve(); b.solve()
            else:
                a.solve(1e-8, 200, 4); b.solve(1e-8, 200, 4)
            return extra + [x for y in bs for x in read(y)]
        finally:
            close(bs)
    counts, _ = both_modes(sequence)
    assert counts["aux"] == 0 and counts["excluded"] == 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("owner", ["first", "last"])
def test_the_batch_that_owns_the_stream_may_go_first_or_last(n, owner):
    def sequence():
        lead, b1, b2 = bs = family(n, [31, 32, 33], materialised=(1,))
        out = []
        try:
            lead.solve(); b1.solve(); b2.solve(); lead.solve()
            if owner == "first":
                out += read(lead)
                b1.solve(); b2.solve()
                lead.close()      # with solves of its borrowers still pending: the stream lives on until the last of them is gone
                b2.solve()
            out += read(b1) + read(b2)
            if owner == "last":
                b1.close()
                b2.close()
                out += read(lead)
            return out
        finally:
            close(bs)
    counts, _ = both_modes(sequence)
    assert counts["aux"] >= 2


@pytest.mark.parametrize("n", SIZES)
def test_two_owner_streams_get_two_contexts(n):
    rp.solve_overlap(2)
    one, two = family(n, [41, 42]), family(n, [43, 44])
    try:
        before = rp.solve_overlap_stats()["aux"]
        one[0].solve(); two[0].solve()      # the first solve of EACH stream stays on it: the second call does not alternate with the first
        assert rp.solve_overlap_stats()["aux"] == before
        one[1].solve(); two[1].solve()      # ... and each stream's second solve goes beside its first
        assert rp.solve_overlap_stats()["aux"] == before + 2
        got = [x for b in one + two for x in read(b)]
    finally:
        close(one)
        close(two)

    def serial():
        bs = family(n, [41, 42, 43, 44])
        try:
            for b in bs:
                b.solve()
            return [x for b in bs for x in read(b)]
        finally:
            close(bs)
    ref, _ = run(0, serial)
    assert all(r.tobytes() == g.tobytes() for r, g in zip(ref, got))


def test_small_batches_are_left_alone_by_default():
    def sequence():
        bs = family(1000, [51, 52, 53, 54])
        try:
            for b in bs:
                b.solve()
            return [x for b in bs for x in read(b)]
        finally:
            close(bs)
    ref, idle = run(0, sequence)
    assert idle == {"aux": 0, "kept": 0, "joins": 0, "excluded": 0}
    got, counts = run(1, sequence)
    assert counts["aux"] == 0 and counts["joins"] == 0 and counts["kept"] == 4
    assert all(r.tobytes() == g.tobytes() for r, g in zip(ref, got))
