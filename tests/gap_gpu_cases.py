"""The cases of tests/test_gpu_gap.py, each run in a fresh process (`python tests/gap_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound is
what it is: DESIGN.md section 18."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_ref as gr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV = tg.DEV
N = 300                # three trips at 128 problems per trip, the last one partial
SHAPES = ((N, 1), (N, 7), (N - 1, 7), (N, 8))      # 299 x 7 is an odd total: the single trailing query of stream_pairs
LD = np.longdouble
FAMILIES = ("random", "solved", "follower", "follower0", "knot")
NAMES = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")
BOTH = (True, True)
_t, _bits, _same_bits, _head, Out = tg._t, tg._bits, tg._same_bits, tg._head, tg.Out


def _golden_positions(n):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f3_batch.npz"))
    return z["pos"][:n].copy()


def _device_solve(pos):
    """The spline the device's gated solve leaves for rest-to-rest problems at the positions (n, 3)."""
    n = len(pos)
    with rp.Batch(n) as b:
        ts = [_t(pos[:, c]) for c in range(3)]
        b.set_problems_device(*[t.data_ptr() for t in ts])
        b.solve(1e-8, 200, 0)
        sp = tr.spline_of_state(b.get_state())
    assert np.isfinite(np.stack(sp)).all() and np.all(sp[6] > 0) and np.all(sp[7] > 0)
    return sp


def _family(name, n=N):
    """(A, B, the family's delays for k columns as a function of (k, seed)): gap_ref's pairs; the solved ones are a device solve of the
    golden file's positions, problems [0, N) against [N, 2 N), and the follower is the solved A 25 lower."""
    if name == "knot":
        a, b, _, _, delay, _ = gr.knot_cases()
        return a, b, lambda k, seed: np.repeat(delay, k, axis=1)
    if name == "random":
        a, b = gr.random_pair(N)
    else:
        both = _device_solve(_golden_positions(2 * N))
        a, b = [x[:N].copy() for x in both], [x[N:].copy() for x in both]
        if name != "solved":
            b = gr.follower(a)
    a, b = _head(a, n), _head(b, n)
    if name == "follower0":
        return a, b, lambda k, seed: np.zeros((n, k))
    return a, b, lambda k, seed: gr.delays(a, b, k, seed, follow=name == "follower")


def _queries(name, a, b, delays, k, seed):
    delay = delays(k, seed)
    if name == "knot":      # the whole common domain in every column
        return np.full(delay.shape, -np.inf), np.full(delay.shape, np.inf), delay
    lo, hi = gr.windows(a, b, delay, seed + 1)
    return lo, hi, delay


def _gap(a, b, lo, hi, delay, k=None, values=BOTH, times=BOTH, zero_vel=False):
    """The stateless entry: (two values, two times), None where not asked for.  lo / hi / delay of None go in as NULL."""
    n = len(a[0])
    k = k if k is not None else next(x for x in (lo, hi, delay) if x is not None).shape[1]
    ta, tb = [_t(x) for x in a], [_t(x) for x in b]
    tl, th, td = (_t(x) if x is not None else None for x in (lo, hi, delay))
    outs = [Out(n, k) if w else None for w in tuple(values) + tuple(times)]
    addr_a, addr_b = [t.data_ptr() for t in ta], [t.data_ptr() for t in tb]
    if zero_vel:
        addr_a[3] = addr_a[4] = addr_b[3] = addr_b[4] = 0
    ptr = [o.ptr if o else 0 for o in outs]
    capi.trajectory_gap(0, 0, n, k, addr_a, addr_b, *[t.data_ptr() if t is not None else 0 for t in (tl, th, td)], ptr[:2], ptr[2:])
    torch.cuda.synchronize()
    got = [o.get() if o else None for o in outs]
    return got[:2], got[2:]


def _all_same(x, y):
    return all(_same_bits(p, q) for p, q in zip(x[0] + x[1], y[0] + y[1]))


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    """The CPU test's tolerances and caps: NaN mask identical, values within 2e-13 of the scale, times off ties within 1e-12 of
    max(T_A, T_B), at most 1 % (solved: 10 %) of the queries left out of the time comparison; the follower with no delay: 25 to the value
    bound, times left out; the hand-made cases exact."""
    worst = {"value, of the scale": 0.0, "time off ties, of max(T_A, T_B)": 0.0, "left out": 0.0}
    shapes = ((4, 1), (4, 7), (4, 8)) if family == "knot" else SHAPES
    for n, k in shapes:
        a, b, delays = _family(family, n)
        sc, T = gr.scale(a, b), np.maximum(a[6] + a[7], b[6] + b[7])[:, None]
        lo, hi, delay = _queries(family, a, b, delays, k, 300 + k)
        want_v, want_t = gr.gap_ld(a, b, lo, hi, delay)
        gap = gr.runner_up_gap(a, b, lo, hi, delay)
        got_v, got_t = _gap(a, b, lo, hi, delay)
        for j, name in enumerate(gr.NAMES):
            missing = np.isnan(want_v[j])
            assert np.array_equal(np.isnan(got_v[j]), missing) and np.array_equal(np.isnan(got_t[j]), missing), (family, n, k, name, "the NaN mask")
            err = float(np.where(missing, 0, np.abs(got_v[j] - want_v[j]) / sc).max())
            worst["value, of the scale"] = max(worst["value, of the scale"], err)
            if family == "follower0":
                assert float(np.where(missing, 0, np.abs(got_v[j] - 25.0) / sc).max()) <= 2e-13, (n, k, name)
                continue
            clear = ~missing & (gap[j] >= 1e-9)
            terr = float(np.where(clear, np.abs(got_t[j] - want_t[j]) / T, 0).max())
            worst["time off ties, of max(T_A, T_B)"] = max(worst["time off ties, of max(T_A, T_B)"], terr)
            left = float((~missing & ~clear).sum() / max((~missing).sum(), 1))
            worst["left out"] = max(worst["left out"], left)
            print("%s %d x %d %s: value %.2e of the scale, time off ties %.2e, %.2f %% left out" % (family, n, k, name, err, terr, 100 * left))
            if k > 1 and family != "knot":      # one column is one whole-domain query per problem: the cap is the CPU test's, for its eight columns
                assert left <= (0.10 if family == "solved" else 0.01), (family, n, k, name, left)
        if family == "knot":
            for i, (j, value, time, cls) in enumerate(gr.knot_cases()[5]):
                assert np.all(got_v[j][i] == value) and np.all(got_t[j][i] == time), (i, got_v[j][i], got_t[j][i])
                assert np.all(gr.classes(a, b, lo, hi, delay, got_t[j])[i] == cls), i
        # a NULL window end is the infinite one and a NULL delay zeros, bit for bit
        full = (got_v, got_t)
        inf, zero = np.full(lo.shape, np.inf), np.zeros(lo.shape)
        assert _all_same(_gap(a, b, None, hi, delay), _gap(a, b, -inf, hi, delay)) and _all_same(_gap(a, b, lo, None, delay), _gap(a, b, lo, inf, delay)), (family, k)
        assert _all_same(_gap(a, b, lo, hi, None), _gap(a, b, lo, hi, zero)) and _all_same(_gap(a, b, None, None, None, k=k), _gap(a, b, -inf, inf, zero)), (family, k)
        if k == 7:
            # every output alone, and every output alone left out: the others' bits do not change, and nothing else is written
            for f in range(4):
                for alone in (True, False):
                    want = [(g == f) == alone for g in range(4)]
                    some = _gap(a, b, lo, hi, delay, values=want[:2], times=want[2:])
                    for g, x in enumerate(some[0] + some[1]):
                        assert (x is None) == (not want[g]) and (x is None or _same_bits(x, (full[0] + full[1])[g])), (family, f, alone, g)
    print("%s: %s" % (family, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["value, of the scale"] <= 2e-13 and worst["time off ties, of max(T_A, T_B)"] <= 1e-12
    if family != "random":
        return
    # the NaN rule: a duration of 0, -1, inf, NaN in either spline poisons its problem and no other; a NaN window end, a NaN or infinite
    # delay its own query and no other
    a, b, delays = _family(family, 257)
    lo, hi, delay = _queries(family, a, b, delays, 7, 1)
    clean = _gap(a, b, lo, hi, delay)
    a, b = [x.copy() for x in a], [x.copy() for x in b]
    a[6][3], b[7][64], a[6][130], b[7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    delay[12, 1], delay[13, 2], delay[14, 3] = np.nan, np.inf, -np.inf
    bad = np.zeros((257, 7), dtype=bool)
    bad[[3, 64, 130, 256]] = True
    bad[10, 0] = bad[200, 4] = bad[11, 3] = bad[12, 1] = bad[13, 2] = bad[14, 3] = True
    got = _gap(a, b, lo, hi, delay)
    for x, ref in zip(got[0] + got[1], clean[0] + clean[1]):
        assert np.array_equal(np.isnan(x), bad | np.isnan(ref))
        assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad]))
    # NULL end velocities are zeros
    za, zb = [x.copy() for x in a], [x.copy() for x in b]
    for s in (za, zb):
        s[3][:], s[4][:] = 0.0, 0.0
    assert _all_same(_gap(za, zb, lo, hi, delay, zero_vel=True), _gap(za, zb, lo, hi, delay))


# ---------------------------------------------------------------- 2. the invariant
def test_every_value_is_the_difference_of_the_evaluators_at_the_returned_time():
    for family in FAMILIES:
        for n, k in SHAPES[1:] if family != "knot" else ((4, 7),):
            a, b, delays = _family(family, n)
            lo, hi, delay = _queries(family, a, b, delays, k, 400 + k)
            values, times = _gap(a, b, lo, hi, delay)
            for j in range(2):
                missing = np.isnan(times[j])
                at = np.where(missing, 0.0, times[j])
                out = tg._eval(a, at, want=(True, False, False))[0] - tg._eval(b, at - np.where(missing, 0.0, delay), want=(True, False, False))[0]
                assert np.array_equal(np.isnan(values[j]), missing), (family, n, k, gr.NAMES[j])
                assert np.array_equal(_bits(out[~missing]), _bits(values[j][~missing])), (family, n, k, gr.NAMES[j])
    print("every value is rp_trajectory_eval(A, t) - rp_trajectory_eval(B, t - delay) at the returned time, bit for bit")


# ---------------------------------------------------------------- 3. reproducibility
def test_bits_depend_on_the_problem_and_its_query_only():
    for family in ("random", "solved", "follower"):
        a, b, delays = _family(family)
        lo, hi, delay = _queries(family, a, b, delays, 7, 507)
        first = _gap(a, b, lo, hi, delay)
        assert _all_same(first, _gap(a, b, lo, hi, delay)), "differs from run to run"
        # the problems in another order
        order = np.random.default_rng(5).permutation(N)
        moved = _gap([x[order] for x in a], [x[order] for x in b], lo[order], hi[order], delay[order])
        assert _all_same(moved, ([x[order] for x in first[0]], [x[order] for x in first[1]])), family
        # batches of their own: one problem, one trip and a problem, the last trip alone
        for rows in (slice(0, 1), slice(0, 129), slice(256, N)):
            own = _gap([x[rows] for x in a], [x[rows] for x in b], lo[rows], hi[rows], delay[rows])
            assert _all_same(own, ([x[rows] for x in first[0]], [x[rows] for x in first[1]])), (family, rows)
        # the seven columns inside a launch of eight: every query lands in another thread, next to another query
        for at in (0, 3, 7):
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=1))      # noqa: E731
            eight = _gap(a, b, wide(lo, 0.1), wide(hi, 0.2), wide(delay, 0.05))
            assert _all_same(([np.delete(x, at, axis=1) for x in eight[0]], [np.delete(x, at, axis=1) for x in eight[1]]), first), (family, at)
    print("the same bits in any order, in any batch and in any launch shape")


# ---------------------------------------------------------------- 4. autograd
def _leaves(a, b, lo, hi, delay):
    ins_a = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, a)}
    ins_b = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, b)}
    return ins_a, ins_b, [_t(x).requires_grad_() for x in (lo, hi, delay)]


def _run(va, vb, lo, hi, delay):
    six = lambda v: [v[nm] for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1", "vel0", "vel2")]      # noqa: E731
    return rp.trajectory_gap(six(va), six(vb), lo, hi, delay)


def test_autograd_reverse_forward_and_duality():
    k = 7
    for family in ("random", "solved", "follower"):
        a, b, delays = _family(family)
        lo_np, hi_np, dl_np = _queries(family, a, b, delays, k, 8)
        ins_a, ins_b, (lo, hi, delay) = _leaves(a, b, lo_np, hi_np, dl_np)
        rng = np.random.default_rng(9)
        g = [_t(rng.standard_normal((N, k))) for _ in range(2)]
        outs = _run(ins_a, ins_b, lo, hi, delay)
        assert len(outs) == 4 and not any(o.requires_grad for o in outs[2:]) and all(o.requires_grad for o in outs[:2])
        dev_v, dev_t = _gap(a, b, lo_np, hi_np, dl_np)
        assert all(_same_bits(o.detach().cpu().numpy(), x) for o, x in zip(outs, dev_v + dev_t)), family
        leaves = [ins_a[nm] for nm in NAMES] + [ins_b[nm] for nm in NAMES] + [lo, hi, delay]
        got = [x.cpu().numpy() for x in torch.autograd.grad(outs[:2], leaves, grad_outputs=g, retain_graph=True)]
        miss = np.isnan(dev_v[0]) | np.isnan(dev_v[1])
        assert all(np.isfinite(x).all() for x in got) and all(np.all(x[miss] == 0) for x in got[16:]), family
        cls = np.concatenate([gr.classes(a, b, lo_np, hi_np, dl_np, t) for t in dev_t], axis=1)
        shares = np.bincount(cls.ravel(), minlength=9) / cls.size
        print("%s: classes of the returned times: LO %.3f HI %.3f END_A %.3f END_B %.3f KNOT_A %.3f KNOT_B %.3f START %.3f interior %.3f none %.3f"
              % ((family,) + tuple(shares)))
        # against the longdouble routing at the device's own times; the yardstick is the same routing on the evaluator's float64 restatement
        gn = [x.cpu().numpy() for x in g]
        flat = lambda r: list(r[0]) + list(r[1]) + [r[2], r[3], r[4]]      # noqa: E731
        ref = flat(gr.derivative_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, gn))
        r64 = flat(gr.derivative_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, gn, vjp=tr.vjp_f64))
        restated, device = float(np.max(tr.normwise(r64, ref))), float(np.max(tr.normwise(got, ref)))
        print("%s: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # forward mode
        da, db = [_t(d) for d in tg._tangents(N, k, 10)[0]], [_t(d) for d in tg._tangents(N, k, 11)[0]]
        q_dot = [_t(rng.standard_normal((N, k))) for _ in range(3)]
        with fwAD.dual_level():
            dual_a = {nm: fwAD.make_dual(ins_a[nm].detach(), d) for nm, d in zip(NAMES, da)}
            dual_b = {nm: fwAD.make_dual(ins_b[nm].detach(), d) for nm, d in zip(NAMES, db)}
            douts = _run(dual_a, dual_b, *[fwAD.make_dual(x.detach(), d) for x, d in zip((lo, hi, delay), q_dot)])
            got_dot = [fwAD.unpack_dual(o).tangent.cpu().numpy() for o in douts[:2]]
            assert all(fwAD.unpack_dual(o).tangent is None for o in douts[2:])

        def f(*xs):
            return _run(dict(zip(NAMES, xs[:8])), dict(zip(NAMES, xs[8:16])), *xs[16:])[:2]
        _, func_dot = torch.func.jvp(f, tuple(x.detach() for x in leaves), tuple(da) + tuple(db) + tuple(q_dot))
        assert all(_same_bits(x.cpu().numpy(), y) for x, y in zip(func_dot, got_dot)), family
        assert all(np.array_equal(np.isnan(x), miss) for x in got_dot), family
        dan, dbn, qn = [d.cpu().numpy() for d in da], [d.cpu().numpy() for d in db], [d.cpu().numpy() for d in q_dot]
        zap = lambda xs: [np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x) for x in xs]      # noqa: E731
        dot_ld = zap(gr.derivative_jvp_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, dan, dbn, *qn))
        dot64 = zap(gr.derivative_jvp_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, dan, dbn, *qn, jvp=tr.jvp_f64))
        restated, device = float(np.max(tr.normwise(dot64, dot_ld))), float(np.max(tr.normwise(zap(got_dot), dot_ld)))
        print("%s: forward mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # duality between the two modes: <g, J u> = <J^T g, u>
        left_terms = [np.where(np.isnan(d), 0, x.astype(LD) * d) for x, d in zip(gn, got_dot)]
        right_terms = [x.astype(LD) * d for x, d in zip(got, dan + dbn + qn)]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        size = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, family
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(_run(ins_a, ins_b, lo, hi, delay)[1]) ** 2).sum(), ins_a["pos1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        if family != "random":
            continue
        # a (k,) query is every problem's; all three None: k = 1, the whole common domain; six tensors: vel0 / vel2 are zeros
        z = np.zeros(N)
        flat_a, flat_b = [a[0], a[1], a[2], z, z, a[5], a[6], a[7]], [b[0], b[1], b[2], z, z, b[5], b[6], b[7]]
        six_a = [ins_a[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        six_b = [ins_b[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        row = np.array([0.01, -0.02, 0.0])
        row_delay = _t(row).requires_grad_()
        o = rp.trajectory_gap(six_a, six_b, None, None, row_delay)
        want = _gap(flat_a, flat_b, None, None, np.repeat(row[None, :], N, axis=0))
        assert all(_same_bits(x.detach().cpu().numpy(), y) for x, y in zip(o, want[0] + want[1]))
        (g_row,) = torch.autograd.grad(torch.nan_to_num(o[0]).sum(), row_delay)
        assert g_row.shape == (3,)
        whole = rp.trajectory_gap(six_a, six_b)
        want = _gap(flat_a, flat_b, None, None, None, k=1)
        assert whole[0].shape == (N, 1) and all(_same_bits(x.cpu().numpy(), y) for x, y in zip(whole, want[0] + want[1]))
    # the hand-made cases: the delay's gradient through the KNOT_A, KNOT_B, START and END_B routes, exactly
    a, b, lo_np, hi_np, dl_np, want = gr.knot_cases()
    ins_a, ins_b, (lo, hi, delay) = _leaves(a, b, lo_np, hi_np, dl_np)
    outs = _run(ins_a, ins_b, lo, hi, delay)
    leaves = [ins_a[nm] for nm in NAMES] + [ins_b[nm] for nm in NAMES] + [lo, hi, delay]
    slopes = (8.0, 8.0, -56.25, 45.0)      # d value / d delay: the velocity of A (cases 2, 3) or of B (cases 0, 1) at the returned time
    for i, (j, value, time, cls) in enumerate(want):
        assert outs[j][i, 0].item() == value and outs[2 + j][i, 0].item() == time, i
        gr_i = [x.cpu().numpy() for x in torch.autograd.grad(outs[j][i, 0], leaves, retain_graph=True)]
        print("hand-made case %d (class %d): d / d delay %.17g, d / d lo %.17g, d / d hi %.17g" % (i, cls, gr_i[18][i, 0], gr_i[16][i, 0], gr_i[17][i, 0]))
        assert gr_i[18][i, 0] == slopes[i] and gr_i[16][i, 0] == 0 and gr_i[17][i, 0] == 0, (i, gr_i[18][i, 0])
        assert all(np.all(np.delete(x, i, axis=0) == 0) for x in gr_i), i
        onehot = torch.zeros_like(delay)
        onehot[i, 0] = 1.0
        with fwAD.dual_level():
            d = _run({nm: t.detach() for nm, t in ins_a.items()}, {nm: t.detach() for nm, t in ins_b.items()}, lo.detach(), hi.detach(),
                     fwAD.make_dual(delay.detach(), onehot))
            assert fwAD.unpack_dual(d[j]).tangent[i, 0].item() == slopes[i], i
    # END_B: the gap's maximum is A at delay + T_B minus pos2 of B: it moves with B's two durations as with the delay, and with pos2 by -1
    end = [x.cpu().numpy() for x in torch.autograd.grad(outs[1][3, 0], leaves, retain_graph=True)]
    print("END_B: d / d (B's pos2, duration0, duration1) = %.17g, %.17g, %.17g" % (end[8 + 2][3], end[8 + 6][3], end[8 + 7][3]))
    assert abs(end[8 + 2][3] + 1.0) <= 1e-12 and abs(end[8 + 6][3] - 45.0) <= 45.0 * 1e-12 and abs(end[8 + 7][3] - 45.0) <= 45.0 * 1e-12
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. through the solves
def test_the_pipeline_against_central_differences():
    """min_time_gap on the delayed follower family against central differences of itself in pos1 of each vehicle, on converged finite
    queries whose winner leads by 1e-2 of the scale: section 15's pipeline bound, median < 1e-5 and 95 % < 1e-3."""
    n, k = N, 8
    pos = _golden_positions(n)
    xa = [_t(pos[:, c]).requires_grad_() for c in range(3)]
    xb = [_t(pos[:, c] - 25.0).requires_grad_() for c in range(3)]

    def pipeline(pa, pb, lo, hi, delay):
        return rp.min_time_gap(pa, pb, lo, hi, delay, gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(xa, xb, None, None, None)
    assert len(first) == 6 and len(first[4]) == 5 and len(first[5]) == 5
    sols = [[t.cpu().numpy() for t in s[:3]] for s in first[4:]]
    conv = np.ones(n, dtype=bool)
    for s, status in zip(sols, (first[4][4], first[5][4])):
        conv &= np.isfinite(np.stack(s, 1)).all(1) & (s[1] > 0) & (s[2] > 0) & ((status & capi.ST_CONVERGED) != 0).cpu().numpy()
    print("%d of %d pairs converged" % (int(conv.sum()), n))
    assert conv.mean() > 0.95
    z = np.zeros(n)
    a = [np.where(conv, x, 1.0) for x in (pos[:, 0], pos[:, 1], pos[:, 2], z, z) + tuple(sols[0])]
    b = [np.where(conv, x, 1.0) for x in (pos[:, 0] - 25, pos[:, 1] - 25, pos[:, 2] - 25, z, z) + tuple(sols[1])]
    dl_np = gr.delays(a, b, k, 23, follow=True)      # fixed times: the queries do not move with the solutions
    lo_np, hi_np = gr.windows(a, b, dl_np, 24)
    lo, hi, delay = _t(lo_np), _t(hi_np), _t(dl_np)
    out = pipeline(xa, xb, lo, hi, delay)
    gap = gr.runner_up_gap(a, b, lo_np, hi_np, dl_np)
    wt = _t(np.random.default_rng(25).uniform(0.5, 1.5, (n, k)))
    h = 1e-4
    moved = {}
    with torch.no_grad():
        for which in range(2):
            up, dn = [list(xa), list(xb)], [list(xa), list(xb)]
            up[which][1], dn[which][1] = up[which][1] + h, dn[which][1] - h
            moved[which] = (pipeline(up[0], up[1], lo, hi, delay)[:2], pipeline(dn[0], dn[1], lo, hi, delay)[:2])
    for j, name in enumerate(gr.NAMES):
        finite = conv[:, None] & np.isfinite(out[j].detach().cpu().numpy())
        keep_np = finite & (gap[j] >= 1e-2)
        share = keep_np.sum() / finite.sum()
        keep = _t(keep_np).bool()
        rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
        grads = torch.autograd.grad(rows(out[j]).sum(), [xa[1], xb[1]], retain_graph=True)
        some = _t(keep_np.any(axis=1)).bool()
        print("%s: %.0f %% of the converged, finite queries lead by 1e-2 of the scale, in %.0f %% of the problems" % (name, 100 * share, 100 * float(some.float().mean())))
        for which, vehicle in enumerate("ab"):
            fd = (rows(moved[which][0][j]) - rows(moved[which][1][j])) / (2 * h)
            ok = some & torch.isfinite(fd) & torch.isfinite(grads[which])
            rel = ((grads[which] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]
            print("  d %s / d pos1 of %s against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% of the problems)"
                  % (name, vehicle, rel.median(), rel.quantile(0.95), 100 * float(ok.float().mean())))
            assert float(ok.float().mean()) > 0.5 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, (name, vehicle)
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
