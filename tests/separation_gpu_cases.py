"""The cases of tests/test_gpu_separation.py, each run in a fresh process (`python tests/separation_gpu_cases.py <case> [family] [d]`), on
top of tests/trajectory_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each
bound is what it is: DESIGN.md section 24."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_gpu_cases as gg  # noqa: E402
import gap_ref as gr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import separation_ref as sr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

N = 300                # three trips at 128 problems per trip (every d stages 128), the last one partial
SHAPES = ((N, 1), (N, 7), (N - 1, 7), (N, 8))      # 299 x 7 is an odd total: the single trailing query of stream_pairs
LD = np.longdouble
SIX = (0, 1, 2, 5, 6, 7, 3, 4)      # the table's order as the torch layer's sequence: pos0, pos1, pos2, vel1, duration0, duration1, vel0, vel2
LEFT_OUT = {"random": 0.01, "solved": 0.10, "follower": 0.01}      # the CPU table's caps on the share left out of the time comparison
_t, _bits, _same_bits, Out = tg._t, tg._bits, tg._same_bits, tg.Out


def _family(name, d, n=N):
    if name == "hand":
        a, b, lo, hi, delay, _ = sr.hand_made()
        return a, b, lambda k, seed: (np.repeat(lo, k, axis=1), np.repeat(hi, k, axis=1), np.repeat(delay, k, axis=1))
    a, b = sr.vehicles(name, N, d)
    a, b = [tg._head(x, n) for x in a], [tg._head(x, n) for x in b]

    def queries(k, seed):
        delay = np.zeros((n, k)) if name == "follower0" else sr.delays(a, b, k, seed, follow=name == "follower")
        lo, hi = sr.windows(a, b, delay, seed + 1)
        return lo, hi, delay
    return a, b, queries


def _sep(a, b, lo, hi, delay, k=None, want=(True, True), zero_vel=False):
    """The stateless entry: (value, time), None where not asked for.  lo / hi / delay of None go in as NULL."""
    n, d = len(a[0][0]), len(a)
    k = k if k is not None else next(x for x in (lo, hi, delay) if x is not None).shape[1]
    ta, tb = [[_t(x) for x in s] for s in a], [[_t(x) for x in s] for s in b]
    tl, th, td = (_t(x) if x is not None else None for x in (lo, hi, delay))
    outs = [Out(n, k) if w else None for w in want]
    addr = lambda v: [0 if zero_vel and f in (3, 4) else t.data_ptr() for s in v for f, t in enumerate(s)]      # noqa: E731
    capi.trajectory_separation(0, 0, n, k, d, addr(ta), addr(tb), *[t.data_ptr() if t is not None else 0 for t in (tl, th, td)],
                               *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _all_same(x, y):
    return all(_same_bits(p, q) for p, q in zip(x, y))


def _rows(v, rows):
    return [[x[rows] for x in s] for s in v]


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family, d):
    """The CPU test's bounds and caps: the NaN mask identical, values within B, f_ld at the returned time within 2 B of the definition's
    minimum, the time's bits exact where the definition's winner is a boundary candidate that leads by 1e-9 of the scale^2, at most the
    CPU table's share left out; the follower with no delay: 625 d to B; the hand-made cases exact."""
    d = int(d)
    worst = {"value, of B": 0.0, "f at the returned time over the minimum, of 2 B": 0.0, "left out": 0.0}
    for n, k in ((4, 1), (4, 7), (4, 8)) if family == "hand" else SHAPES:
        a, b, queries = _family(family, d, n)
        lo, hi, delay = queries(k, 300 + k)
        cand = sr.candidates_ld(a, b, lo, hi, delay)
        want_v, want_t = sr.separation_ld(a, b, candidates=cand)
        lead = sr.runner_up(a, b, candidates=cand)
        got_v, got_t = _sep(a, b, lo, hi, delay)
        missing = np.isnan(np.asarray(want_v, dtype=np.float64))
        assert np.array_equal(np.isnan(got_v), missing) and np.array_equal(np.isnan(got_t), missing), (family, d, n, k, "the NaN mask")
        f_at, gaps = sr.f_ld(a, b, np.where(missing, 0.0, got_t), np.where(missing, 0.0, delay))
        B = sr.value_bound(a, b, gaps)
        err = float(np.where(missing, 0, np.abs(got_v - f_at) / B).max())
        over = float(np.where(missing, 0, (f_at - want_v) / (2 * B)).max())
        worst["value, of B"] = max(worst["value, of B"], err)
        worst["f at the returned time over the minimum, of 2 B"] = max(worst["f at the returned time over the minimum, of 2 B"], over)
        if family == "follower0":
            assert float(np.where(missing, 0, np.abs(got_v - 625.0 * d) / B).max()) <= 1.0, (d, n, k)
        elif family == "hand":
            for i, (value, time, cls, axis) in enumerate(sr.hand_made()[5]):
                assert np.all(got_v[i] == value) and np.all(got_t[i] == time), (i, got_v[i], got_t[i])
                got_cls = sr.classes(a, b, lo, hi, delay, got_t)
                assert np.all(got_cls[0][i] == cls) and np.all(got_cls[1][i] == axis), i
        else:
            cls = sr.classes(a, b, lo, hi, delay, np.asarray(want_t, dtype=np.float64))[0]
            boundary = ~missing & (cls != sr.OTHER)
            clear = boundary & (lead >= 1e-9)
            assert _same_bits(got_t[clear], np.asarray(want_t, dtype=np.float64)[clear]), (family, d, n, k, "the bits of a boundary time")
            left = float((boundary & ~clear).sum() / max(boundary.sum(), 1))
            worst["left out"] = max(worst["left out"], left)
            print("%s d = %d, %d x %d: value %.2e of B, over the minimum %.2e of 2 B, %.2f %% left out" % (family, d, n, k, err, over, 100 * left))
            if k > 1:      # one column is one whole-domain query per problem: the cap is the CPU test's, for its eight columns
                assert left <= (0.15 if d == 1 else LEFT_OUT[family]), (family, d, n, k, left)
        # a NULL window end is the infinite one and a NULL delay zeros, bit for bit
        full = [got_v, got_t]
        inf, zero = np.full(lo.shape, np.inf), np.zeros(lo.shape)
        assert _all_same(_sep(a, b, None, hi, delay), _sep(a, b, -inf, hi, delay)) and _all_same(_sep(a, b, lo, None, delay), _sep(a, b, lo, inf, delay))
        assert _all_same(_sep(a, b, lo, hi, None), _sep(a, b, lo, hi, zero)) and _all_same(_sep(a, b, None, None, None, k=k), _sep(a, b, -inf, inf, zero))
        if k == 7:      # each output alone: the same bits, and nothing else is written (the sentinels behind every output)
            for f in range(2):
                some = _sep(a, b, lo, hi, delay, want=[g == f for g in range(2)])
                assert some[1 - f] is None and _same_bits(some[f], full[f]), (family, d, f)
    print("%s d = %d: %s" % (family, d, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["value, of B"] <= 1.0 and worst["f at the returned time over the minimum, of 2 B"] <= 1.0
    if family != "random":
        return
    # the NaN rule: a duration of 0, -1, inf, NaN in any one of the 2 d splines poisons its problem and no other; a NaN window end, a NaN
    # or infinite delay its own query and no other
    a, b, queries = _family(family, d, 257)
    lo, hi, delay = queries(7, 1)
    clean = _sep(a, b, lo, hi, delay)
    a, b = [[x.copy() for x in s] for s in a], [[x.copy() for x in s] for s in b]
    a[0][6][3], b[d - 1][7][64], a[d - 1][6][130], b[0][7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    delay[12, 1], delay[13, 2], delay[14, 3] = np.nan, np.inf, -np.inf
    bad = np.zeros((257, 7), dtype=bool)
    bad[[3, 64, 130, 256]] = True
    bad[10, 0] = bad[200, 4] = bad[11, 3] = bad[12, 1] = bad[13, 2] = bad[14, 3] = True
    for x, ref in zip(_sep(a, b, lo, hi, delay), clean):
        assert np.array_equal(np.isnan(x), bad | np.isnan(ref))
        assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad]))
    # NULL end velocities are zeros
    za, zb = [[x.copy() for x in s] for s in a], [[x.copy() for x in s] for s in b]
    for s in za + zb:
        s[3][:], s[4][:] = 0.0, 0.0
    assert _all_same(_sep(za, zb, lo, hi, delay, zero_vel=True), _sep(za, zb, lo, hi, delay))


# ---------------------------------------------------------------- 2. the invariant
def test_every_value_is_the_sum_of_squares_of_the_evaluators_at_the_returned_time():
    for family in ("random", "solved", "follower", "follower0", "hand"):
        for d in (2,) if family == "hand" else (1, 2, 3):
            for n, k in SHAPES[1:3] if family != "hand" else ((4, 7),):
                a, b, queries = _family(family, d, n)
                lo, hi, delay = queries(k, 400 + k)
                value, time = _sep(a, b, lo, hi, delay)
                missing = np.isnan(time)
                at = np.where(missing, 0.0, time)
                total = None
                for x, y in zip(a, b):
                    gap = tg._eval(x, at, want=(True, False, False))[0] - tg._eval(y, at - np.where(missing, 0.0, delay), want=(True, False, False))[0]
                    total = gap * gap if total is None else total + gap * gap
                assert np.array_equal(np.isnan(value), missing), (family, d, n, k)
                assert np.array_equal(_bits(total[~missing]), _bits(value[~missing])), (family, d, n, k)
    print("every value is the sum in axis order of (rp_trajectory_eval(A_c, t) - rp_trajectory_eval(B_c, t - delay))^2 at the returned time, bit for bit")


# ---------------------------------------------------------------- 3. reproducibility
def test_bits_depend_on_the_problem_and_its_query_only():
    for family, d in (("random", 1), ("random", 2), ("random", 3), ("solved", 2), ("follower", 3)):
        a, b, queries = _family(family, d)
        lo, hi, delay = queries(7, 507)
        first = _sep(a, b, lo, hi, delay)
        assert _all_same(first, _sep(a, b, lo, hi, delay)), "differs from run to run"
        order = np.random.default_rng(5).permutation(N)
        assert _all_same(_sep(_rows(a, order), _rows(b, order), lo[order], hi[order], delay[order]), [x[order] for x in first]), (family, d)
        for rows in (slice(0, 1), slice(0, 129), slice(256, N)):      # one problem, one trip and a problem, the last trip alone
            assert _all_same(_sep(_rows(a, rows), _rows(b, rows), lo[rows], hi[rows], delay[rows]), [x[rows] for x in first]), (family, d, rows)
        for at in (0, 3, 7):      # the seven columns inside a launch of eight: every query lands in another thread, next to another query
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=1))      # noqa: E731
            eight = _sep(a, b, wide(lo, 0.1), wide(hi, 0.2), wide(delay, 0.05))
            assert _all_same([np.delete(x, at, axis=1) for x in eight], first), (family, d, at)
    print("the same bits in any order, in any batch and in any launch shape")


# ---------------------------------------------------------------- 4. one axis against the gap
def test_one_axis_against_the_gap_entry():
    """d = 1: the least squared distance is 0 where gap_min <= 0 <= gap_max, else min(gap_min^2, gap_max^2) of rp_trajectory_gap on the same
    inputs, to B."""
    worst = 0.0
    for family in ("random", "solved", "follower"):
        for n, k in SHAPES[1:]:
            a, b, queries = _family(family, 1, n)
            lo, hi, delay = queries(k, 600 + k)
            value, time = _sep(a, b, lo, hi, delay)
            (g_min, g_max), _ = gg._gap(a[0], b[0], lo, hi, delay)
            missing = np.isnan(g_min)
            assert np.array_equal(np.isnan(value), missing), (family, n, k)
            want = np.where((g_min <= 0) & (0 <= g_max), 0.0, np.minimum(g_min * g_min, g_max * g_max))
            near = np.where(np.abs(g_min) < np.abs(g_max), g_min, g_max)
            B = sr.value_bound(a, b, [np.where((g_min <= 0) & (0 <= g_max), 0.0, near)])
            worst = max(worst, float(np.where(missing, 0, np.abs(value - want) / B).max()))
    print("d = 1 against rp_trajectory_gap: %.3g of B" % worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- 5. autograd
def _leaves(a, b, lo, hi, delay):
    """(A's and B's leaves as (n, d) tensors in the table's order, the three query leaves)"""
    stack = lambda v: [_t(np.stack([s[f] for s in v], axis=1)).requires_grad_() for f in range(8)]      # noqa: E731
    return stack(a), stack(b), [_t(x).requires_grad_() for x in (lo, hi, delay)]


def _run(va, vb, lo, hi, delay):
    return rp.trajectory_separation([va[f] for f in SIX], [vb[f] for f in SIX], lo, hi, delay)


def _flat(bars_a, bars_b, rest):
    """the restatement's gradients in the leaves' order and shapes"""
    return [np.stack([s[f] for s in v], axis=1) for v in (bars_a, bars_b) for f in range(8)] + list(rest)


def test_autograd_reverse_forward_and_duality():
    k = 7
    for family, d in (("random", 1), ("random", 2), ("random", 3), ("solved", 2), ("follower", 2)):
        a, b, queries = _family(family, d)
        lo_np, hi_np, dl_np = queries(k, 8)
        va, vb, (lo, hi, delay) = _leaves(a, b, lo_np, hi_np, dl_np)
        rng = np.random.default_rng(9)
        g = _t(rng.standard_normal((N, k)))
        outs = _run(va, vb, lo, hi, delay)
        assert len(outs) == 2 and outs[0].requires_grad and not outs[1].requires_grad
        dev_v, dev_t = _sep(a, b, lo_np, hi_np, dl_np)
        assert _same_bits(outs[0].detach().cpu().numpy(), dev_v) and _same_bits(outs[1].cpu().numpy(), dev_t), (family, d)
        leaves = va + vb + [lo, hi, delay]
        got = [x.cpu().numpy() for x in torch.autograd.grad(outs[0], leaves, grad_outputs=g, retain_graph=True)]
        miss = np.isnan(dev_v)
        assert all(np.isfinite(x).all() for x in got) and all(np.all(x[miss] == 0) for x in got[16:]), (family, d)      # a NaN value: exactly 0
        cls = sr.classes(a, b, lo_np, hi_np, dl_np, dev_t)[0]
        print("%s d = %d: classes of the returned times: LO %.3f HI %.3f END_A %.3f END_B %.3f START %.3f other %.3f none %.3f"
              % ((family, d) + tuple(np.bincount(cls.ravel(), minlength=7) / cls.size)))
        # against the longdouble routing at the device's own times; the yardstick is the same routing on the evaluator's float64 restatement
        gn = g.cpu().numpy()
        flat = lambda r: _flat(r[0], r[1], r[2:])      # noqa: E731
        ref = flat(sr.derivative_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, gn))
        r64 = flat(sr.derivative_ld(a, b, lo_np, hi_np, dl_np, dev_t, dev_v, gn, vjp=tr.vjp_f64, forward=tr.forward_f64))
        restated, device = float(np.max(tr.normwise(r64, ref))), float(np.max(tr.normwise(got, ref)))
        print("%s d = %d: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e"
              % (family, d, restated, device, 10 * restated))
        assert device <= 10 * restated, (family, d)
        # forward mode
        dots = [_t(rng.standard_normal((N, d))) for _ in range(16)]
        q_dot = [_t(rng.standard_normal((N, k))) for _ in range(3)]
        with fwAD.dual_level():
            dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(leaves, dots + q_dot)]
            douts = _run(dual[:8], dual[8:16], *dual[16:])
            got_dot = fwAD.unpack_dual(douts[0]).tangent.cpu().numpy()
            assert fwAD.unpack_dual(douts[1]).tangent is None

        def f(*xs):
            return _run(list(xs[:8]), list(xs[8:16]), *xs[16:])[0]
        _, func_dot = torch.func.jvp(f, tuple(x.detach() for x in leaves), tuple(dots + q_dot))
        assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss), (family, d)
        dn = [t.cpu().numpy() for t in dots + q_dot]
        split = lambda ts: [[t[:, c] for t in ts] for c in range(d)]      # noqa: E731
        zap = lambda x: np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x)      # noqa: E731
        args = (a, b, lo_np, hi_np, dl_np, dev_t, dev_v, split(dn[:8]), split(dn[8:16])) + tuple(dn[16:])
        dot_ld = zap(sr.derivative_jvp_ld(*args))
        dot64 = zap(sr.derivative_jvp_ld(*args, jvp=tr.jvp_f64, forward=tr.forward_f64))
        restated, device = float(np.max(tr.normwise([dot64], [dot_ld]))), float(np.max(tr.normwise([zap(got_dot)], [dot_ld])))
        print("%s d = %d: forward mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e"
              % (family, d, restated, device, 10 * restated))
        assert device <= 10 * restated, (family, d)
        # duality between the two modes: <g, J u> = <J^T g, u>
        left_terms = [np.where(np.isnan(got_dot), 0, gn.astype(LD) * got_dot)]
        right_terms = [x.astype(LD) * t for x, t in zip(got, dn)]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        size = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        print("%s d = %d: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, d, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, (family, d)
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(_run(va, vb, lo, hi, delay)[0]) ** 2).sum(), va[1], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        if (family, d) != ("random", 1):
            continue
        # (n,) tensors mean d = 1; a (k,) query is every problem's; all three None: k = 1, the whole common domain; six tensors: vel0 / vel2 zeros
        z = np.zeros(N)
        flat_a, flat_b = [[x[0], x[1], x[2], z, z, x[5], x[6], x[7]] for x in a], [[x[0], x[1], x[2], z, z, x[5], x[6], x[7]] for x in b]
        six_a, six_b = [va[f].detach()[:, 0].contiguous() for f in SIX[:6]], [vb[f].detach()[:, 0].contiguous() for f in SIX[:6]]
        row = np.array([0.01, -0.02, 0.0])
        row_delay = _t(row).requires_grad_()
        o = rp.trajectory_separation(six_a, six_b, None, None, row_delay)
        assert _all_same([x.detach().cpu().numpy() for x in o], _sep(flat_a, flat_b, None, None, np.repeat(row[None, :], N, axis=0)))
        (g_row,) = torch.autograd.grad(torch.nan_to_num(o[0]).sum(), row_delay)
        assert g_row.shape == (3,)
        whole = rp.trajectory_separation(six_a, six_b)
        assert whole[0].shape == (N, 1) and _all_same([x.cpu().numpy() for x in whole], _sep(flat_a, flat_b, None, None, None, k=1))
    # the hand-made cases: the routes of the START and of END_B of axis 0, in closed form (tests/separation_ref.py's hand_made)
    a, b, lo_np, hi_np, dl_np, want = sr.hand_made()
    va, vb, (lo, hi, delay) = _leaves(a, b, lo_np, hi_np, dl_np)
    outs = _run(va, vb, lo, hi, delay)
    leaves = va + vb + [lo, hi, delay]
    # d value / d delay = 2 sum_c D_c vel_Ac(t*) where the time moves with the delay (START, END_B): 2 (4 * 2 + 15.625 * 56.25) and
    # 2 (4 * 2 - 936 * 48); 2 sum_c D_c vel_Bc(t* - delay) where it does not (the knot, the stationary point): 2 (3 * 2 + 32 * 8), 2 (3 * 2 + 31 * 4)
    slopes = (524.0, 1773.8125, -89840.0, 260.0)
    for i, (value, time, cls, axis) in enumerate(want):
        assert outs[0][i, 0].item() == value and outs[1][i, 0].item() == time, i
        gr_i = [x.cpu().numpy() for x in torch.autograd.grad(outs[0][i, 0], leaves, retain_graph=True)]
        print("hand-made case %d (class %d): d / d delay %.17g, d / d lo %.17g, d / d hi %.17g" % (i, cls, gr_i[18][i, 0], gr_i[16][i, 0], gr_i[17][i, 0]))
        assert gr_i[18][i, 0] == slopes[i] and gr_i[16][i, 0] == 0 and gr_i[17][i, 0] == 0, (i, gr_i[18][i, 0])
        assert all(np.all(np.delete(x, i, axis=0) == 0) for x in gr_i), i
        onehot = torch.zeros_like(delay)
        onehot[i, 0] = 1.0
        with fwAD.dual_level():
            dual = _run([t.detach() for t in va], [t.detach() for t in vb], lo.detach(), hi.detach(), fwAD.make_dual(delay.detach(), onehot))
            assert fwAD.unpack_dual(dual[0]).tangent[i, 0].item() == slopes[i], i
    # END_B of axis 0: the window ends with B_0, which runs at a constant 2 -- its two durations move the value as the delay does; pos2 of
    # B_0 by -2 D_0 = -8; A's durations, whose end is not the window's, only through the splines
    end = [x.cpu().numpy() for x in torch.autograd.grad(outs[0][2, 0], leaves, retain_graph=True)]
    print("END_B0: d / d (B_0's pos2, duration0, duration1) = %.17g, %.17g, %.17g" % (end[8 + 2][2, 0], end[8 + 6][2, 0], end[8 + 7][2, 0]))
    assert abs(end[8 + 2][2, 0] + 8.0) <= 8e-12 and abs(end[8 + 6][2, 0] + 89840.0) <= 89840.0 * 1e-12 and abs(end[8 + 7][2, 0] + 89840.0) <= 89840.0 * 1e-12
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. through the solves
def test_the_pipeline_against_central_differences():
    """min_time_separation (d = 2, synchronised) on 300 golden problems per axis against themselves 25 lower on both axes, against central
    differences of itself in pos1 of each vehicle, on converged finite queries whose winner leads by 1e-2 of the query's largest candidate
    value (separation_ref.runner_up, unit="distance"): section 15's
    pipeline bound, median < 1e-5 and 95 % < 1e-3."""
    n, k, d = N, 8, 2
    pos = gg._golden_positions(d * n).reshape(d, n, 3)
    xa = [_t(pos[:, :, c].T).requires_grad_() for c in range(3)]
    xb = [_t(pos[:, :, c].T - 25.0).requires_grad_() for c in range(3)]

    def pipeline(pa, pb, lo, hi, delay):
        return rp.min_time_separation(pa, pb, lo, hi, delay, gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(xa, xb, None, None, None)
    assert len(first) == 4 and len(first[2]) == 5 and len(first[3]) == 5 and all(t.shape == (n, d) for t in first[2] + first[3])
    conv = np.ones(n, dtype=bool)
    vehicles = []
    for x, sol in zip((xa, xb), first[2:]):
        s = [t.cpu().numpy() for t in sol[:3]]
        conv &= (np.isfinite(np.stack(s, 2)).all(2) & (s[1] > 0) & (s[2] > 0) & ((sol[4] & capi.ST_CONVERGED) != 0).cpu().numpy()).all(axis=1)
        stretched, scale = rp.synchronize_axes([t.detach() for t in x] + [t for t in sol[:3]])
        assert float((scale.min(dim=1).values - 1.0).abs().max()) == 0.0
        st = [t.cpu().numpy() for t in stretched]
        z = np.zeros(n)
        vehicles.append([[np.where(conv, v, 1.0) for v in (st[0][:, c], st[1][:, c], st[2][:, c], z, z, st[3][:, c], st[4][:, c], st[5][:, c])]
                         for c in range(d)])
    print("%d of %d pairs converged" % (int(conv.sum()), n))
    assert conv.mean() > 0.95
    a, b = vehicles
    a, b = [[np.where(conv, v, 1.0) for v in s] for s in a], [[np.where(conv, v, 1.0) for v in s] for s in b]
    dl_np = sr.delays(a, b, k, 23, follow=True)      # fixed times: the queries do not move with the solutions
    lo_np, hi_np = sr.windows(a, b, dl_np, 24)
    lo, hi, delay = _t(lo_np), _t(hi_np), _t(dl_np)
    out = pipeline(xa, xb, lo, hi, delay)
    lead = sr.runner_up(a, b, lo_np, hi_np, dl_np, unit="distance")
    wt = _t(np.random.default_rng(25).uniform(0.5, 1.5, (n, k)))
    h = 1e-4
    finite = conv[:, None] & np.isfinite(out[0].detach().cpu().numpy())
    keep_np = finite & (lead >= 1e-2)
    keep = _t(keep_np).bool()
    rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
    grads = torch.autograd.grad(rows(out[0]).sum(), [xa[1], xb[1]])
    some = _t(keep_np.any(axis=1)).bool()
    print("%.0f %% of the converged, finite queries lead by 1e-2 of their largest candidate value, in %.0f %% of the problems" % (100 * keep_np.sum() / finite.sum(), 100 * float(some.float().mean())))
    with torch.no_grad():
        for which, vehicle in enumerate("ab"):
            for c in range(d):
                step = torch.zeros_like(xa[1])
                step[:, c] = h
                up, dn = [list(xa), list(xb)], [list(xa), list(xb)]
                up[which][1], dn[which][1] = up[which][1] + step, dn[which][1] - step
                fd = (rows(pipeline(up[0], up[1], lo, hi, delay)[0]) - rows(pipeline(dn[0], dn[1], lo, hi, delay)[0])) / (2 * h)
                ok = some & torch.isfinite(fd) & torch.isfinite(grads[which][:, c])
                rel = ((grads[which][:, c] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]
                print("  d sep_sq / d pos1 of %s, axis %d, against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% of the problems)"
                      % (vehicle, c, rel.median(), rel.quantile(0.95), 100 * float(ok.float().mean())))
                assert float(ok.float().mean()) > 0.5 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, (vehicle, c)
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
