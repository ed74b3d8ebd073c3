"""The cases of tests/test_gpu_contact.py, each run in a fresh process (`python tests/contact_gpu_cases.py <case> [family] [d]`), on top of
tests/trajectory_gpu_cases.py's and tests/separation_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What
is checked, and why each bound is what it is: DESIGN.md section 25."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import contact_ref as cf  # noqa: E402
import gap_gpu_cases as gg  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import separation_gpu_cases as sg  # noqa: E402
import separation_ref as sr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

N, SHAPES, SIX, LD = sg.N, sg.SHAPES, sg.SIX, np.longdouble
_t, _bits, _same_bits, Out, _rows, _all_same = tg._t, tg._bits, tg._same_bits, tg.Out, sg._rows, sg._all_same


def _con(a, b, level, lo, hi, delay, want_rate=True, zero_vel=False):
    """The stateless entry: (time, rate), rate None where not asked for.  lo / hi / delay of None go in as NULL."""
    n, d, k = len(a[0][0]), len(a), level.shape[1]
    ta, tb = [[_t(x) for x in s] for s in a], [[_t(x) for x in s] for s in b]
    tv, tl, th, td = (_t(x) if x is not None else None for x in (level, lo, hi, delay))
    outs = [Out(n, k), Out(n, k) if want_rate else None]
    addr = lambda v: [0 if zero_vel and f in (3, 4) else t.data_ptr() for s in v for f, t in enumerate(s)]      # noqa: E731
    capi.trajectory_contact(0, 0, n, k, d, addr(ta), addr(tb), *[t.data_ptr() if t is not None else 0 for t in (tv, tl, th, td)],
                            *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _inputs(family, d, n, k, seed):
    """(A, B, level, lo, hi, delay, the definition's sub-pieces) of a family at a shape: the levels are contact_ref.levels on these queries."""
    a, b, queries = sg._family(family, d, n)
    lo, hi, delay = queries(k, seed)
    sub = cf.subpieces_ld(a, b, lo, hi, delay)
    return a, b, cf.levels(a, b, lo, hi, delay, seed + 50, sub)[0], lo, hi, delay, sub


def _bound_c(a, b, t, delay, missing):
    at, dl = np.where(missing, 0.0, t), np.where(missing, 0.0, delay)
    f_at, gaps = sr.f_ld(a, b, at, dl)
    return f_at, sr.value_bound(a, b, gaps) + 4 * cf.EPS * cf.tmax(a, b, delay) * np.abs(np.asarray(cf.rate_ld(a, b, at, dl), dtype=np.float64))


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family, d):
    """The CPU test's conditions: the NaN mask identical, every time inside the definition's sub-piece +- 4 eps Tmax, the residual within
    bound (c); the follower with no delay NaN for any level off 625 d by more than B; the hand-made cases exact."""
    d = int(d)
    if family == "hand":
        return _hand_made()
    worst = 0.0
    for n, k in SHAPES:
        if family == "follower0":
            a, b, queries = sg._family(family, d, n)
            lo, hi, delay = queries(k, 300 + k)
            B = float(np.max(sr.value_bound(a, b, [np.full((n, k), 25.0)] * d)))
            for off in (-2.0 * B - 1.0, 2.0 * B + 1.0, -1e4):
                time, rate = _con(a, b, np.full((n, k), 625.0 * d + off), lo, hi, delay)
                assert np.isnan(time).all() and np.isnan(rate).all(), (d, n, k, off)
            continue
        a, b, level, lo, hi, delay, sub = _inputs(family, d, n, k, 300 + k)
        want, _, (t_lo, t_hi) = cf.contact_ld(a, b, level, lo, hi, delay, subpieces=sub)
        time, rate = _con(a, b, level, lo, hi, delay)
        missing = np.isnan(np.asarray(want, dtype=np.float64))
        assert np.array_equal(np.isnan(time), missing) and np.array_equal(np.isnan(rate), missing), (family, d, n, k, "the NaN mask")
        slack = 4 * cf.EPS * cf.tmax(a, b, delay)
        outside = ~missing & ((time < np.asarray(t_lo, dtype=np.float64) - slack) | (time > np.asarray(t_hi, dtype=np.float64) + slack))
        assert not outside.any(), (family, d, n, k, int(outside.sum()))
        f_at, bound = _bound_c(a, b, time, delay, missing)
        share = float(np.where(missing, 0, np.abs(f_at - level) / bound).max())
        worst = max(worst, share)
        print("%s d = %d, %d x %d: %.1f %% reached, residual %.3f of bound (c)" % (family, d, n, k, 100 * (~missing).mean(), share))
    assert worst <= 1.0


def _hand_made():
    a, b, lo1, hi1, delay1, want = sr.hand_made()
    for k in (1, 7, 8):
        wide = lambda x: np.repeat(x, k, axis=1)      # noqa: E731
        lo, hi, delay = wide(lo1), wide(hi1), wide(delay1)
        least = wide(np.array([[w[0]] for w in want]))
        time, rate = _con(a, b, least, lo, hi, delay)
        for i, (_, t, _, _) in enumerate(want):
            assert np.all(time[i] == t) and not np.signbit(time[i]).any(), (k, i, time[i])
        assert np.all(rate[0] == 0.0) and np.all(rate[3] == 0.0) and np.all(rate[1] != 0.0) and np.all(rate[2] != 0.0), (k, rate)
        time, rate = _con(a, b, least - 1.0, lo, hi, delay)
        assert np.isnan(time).all() and np.isnan(rate).all(), k
        wa = wide(np.array([[0.0], [delay1[1, 0]], [delay1[2, 0]], [0.0]]))
        at_start = np.asarray(sr.f_ld(a, b, wa, delay)[0], dtype=np.float64)
        assert _same_bits(_con(a, b, at_start, lo, hi, delay)[0], wa), k
        inner = wide(np.array([[9.0 + 34.25 ** 2], [0.0], [0.0], [985.5625]]))
        time, _ = _con(a, b, inner, lo, hi, delay)
        missing = np.isnan(time)
        f_at, bound = _bound_c(a, b, time, delay, missing)
        for i in (0, 3):
            assert np.all(np.abs(time[i] - 0.25) <= 4 * cf.EPS * 3.5) and np.all(np.abs(f_at[i] - inner[i]) <= bound[i]), (k, i, time[i])
        assert missing[1].all() and missing[2].all(), k
    print("the hand-made cases: the listed times' bits at the touches, a's bits at f(a), NaN below the minimum, 0.25 inside the first piece")


# ---------------------------------------------------------------- 2. the evaluators
def test_evaluator_consistency():
    """The sum of squares of rp_trajectory_eval's differences at the returned time is the level within bound (c), and d_rate is bit for bit
    2.0 times the sum in axis order from 0.0 of (pos_A - pos_B) (vel_A - vel_B) on its outputs."""
    worst = 0.0
    for family in ("random", "solved", "follower"):
        for d in (1, 2, 3):
            for n, k in SHAPES[1:3]:
                a, b, level, lo, hi, delay, _ = _inputs(family, d, n, k, 400 + k)
                time, rate = _con(a, b, level, lo, hi, delay)
                missing = np.isnan(time)
                at, dl = np.where(missing, 0.0, time), np.where(missing, 0.0, delay)
                total, slope = np.zeros(at.shape), np.zeros(at.shape)
                for x, y in zip(a, b):
                    pa, va, _ = tg._eval(x, at)
                    pb, vb, _ = tg._eval(y, at - dl)
                    total = total + (pa - pb) * (pa - pb)
                    slope = slope + (pa - pb) * (va - vb)
                assert np.array_equal(np.isnan(rate), missing), (family, d, n, k)
                assert np.array_equal(_bits((2.0 * slope)[~missing]), _bits(rate[~missing])), (family, d, n, k)
                _, bound = _bound_c(a, b, time, delay, missing)
                worst = max(worst, float(np.where(missing, 0, np.abs(total - level) / bound).max()))
    print("the evaluators' squared distance at the returned time against the level: %.3f of bound (c); the rate bit for bit" % worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- 3. NULL arguments and the NaN rule
def test_null_arguments_and_the_nan_rule():
    for d in (1, 2, 3):
        a, b, level, lo, hi, delay, _ = _inputs("random", d, 257, 7, 1)
        full = _con(a, b, level, lo, hi, delay)
        inf, zero = np.full(lo.shape, np.inf), np.zeros(lo.shape)
        # a NULL window end is the infinite one and a NULL delay zeros, bit for bit
        assert _all_same(_con(a, b, level, None, hi, delay), _con(a, b, level, -inf, hi, delay)), d
        assert _all_same(_con(a, b, level, lo, None, delay), _con(a, b, level, lo, inf, delay)), d
        assert _all_same(_con(a, b, level, lo, hi, None), _con(a, b, level, lo, hi, zero)), d
        assert _all_same(_con(a, b, level, None, None, None), _con(a, b, level, -inf, inf, zero)), d
        # a NULL d_rate: the same time bits, and nothing else is written (Out.get checks the sentinels behind every output)
        alone = _con(a, b, level, lo, hi, delay, want_rate=False)
        assert alone[1] is None and _same_bits(alone[0], full[0]), d
        # the NaN rule: a duration of 0, -1, inf, NaN in any one of the 2 d splines poisons its problem and no other; a NaN window end, a NaN
        # or infinite delay or level its own query and no other
        sa, sb = [[x.copy() for x in s] for s in a], [[x.copy() for x in s] for s in b]
        lv, l2, h2, dl = level.copy(), lo.copy(), hi.copy(), delay.copy()
        sa[0][6][3], sb[d - 1][7][64], sa[d - 1][6][130], sb[0][7][256] = 0.0, np.inf, -1.0, np.nan
        l2[10, 0], h2[200, 4] = np.nan, np.nan
        dl[12, 1], dl[13, 2], dl[14, 3] = np.nan, np.inf, -np.inf
        lv[15, 0], lv[16, 5], lv[17, 6] = np.nan, np.inf, -np.inf
        bad = np.zeros((257, 7), dtype=bool)
        bad[[3, 64, 130, 256]] = True
        bad[10, 0] = bad[200, 4] = bad[12, 1] = bad[13, 2] = bad[14, 3] = bad[15, 0] = bad[16, 5] = bad[17, 6] = True
        for x, ref in zip(_con(sa, sb, lv, l2, h2, dl), full):
            assert np.array_equal(np.isnan(x), bad | np.isnan(ref)), d
            assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad])), d
        # NULL end velocities are zeros
        za, zb = [[x.copy() for x in s] for s in a], [[x.copy() for x in s] for s in b]
        for s in za + zb:
            s[3][:], s[4][:] = 0.0, 0.0
        assert _all_same(_con(za, zb, level, lo, hi, delay, zero_vel=True), _con(za, zb, level, lo, hi, delay)), d
    print("NULL window ends, delay, rate and end velocities; the NaN rule poisons exactly its problem or its query")


# ---------------------------------------------------------------- 4. reproducibility
def test_bits_depend_on_the_problem_and_its_query_only():
    for family, d in (("random", 1), ("random", 2), ("random", 3), ("solved", 2), ("follower", 3)):
        a, b, level, lo, hi, delay, _ = _inputs(family, d, N, 7, 507)
        first = _con(a, b, level, lo, hi, delay)
        assert _all_same(first, _con(a, b, level, lo, hi, delay)), "differs from run to run"
        order = np.random.default_rng(5).permutation(N)
        assert _all_same(_con(_rows(a, order), _rows(b, order), level[order], lo[order], hi[order], delay[order]), [x[order] for x in first]), (family, d)
        for rows in (slice(0, 1), slice(0, 129), slice(256, N)):      # one problem, one trip and a problem, the last trip alone
            assert _all_same(_con(_rows(a, rows), _rows(b, rows), level[rows], lo[rows], hi[rows], delay[rows]), [x[rows] for x in first]), (family, d, rows)
        for at in (0, 3, 7):      # the seven columns inside a launch of eight: every query lands in another thread, next to another query
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=1))      # noqa: E731
            eight = _con(a, b, wide(level, 1.0), wide(lo, 0.1), wide(hi, 0.2), wide(delay, 0.05))
            assert _all_same([np.delete(x, at, axis=1) for x in eight], first), (family, d, at)
    print("the same bits in any order, in any batch and in any launch shape")


# ---------------------------------------------------------------- 5. the existing entries
def _meet(a, b, level, lo, hi, delay):
    n, k = level.shape
    ts = [[_t(x) for x in s] for s in (a, b)]
    tq = [_t(x) for x in (level, lo, hi, delay)]
    out = Out(n, k)
    capi.trajectory_meeting(0, 0, n, k, [t.data_ptr() for t in ts[0]], [t.data_ptr() for t in ts[1]], *[t.data_ptr() for t in tq], out.ptr, 0)
    torch.cuda.synchronize()
    return out.get()


def test_against_the_existing_entries():
    """Where f(a) > level: d = 1 against rp_trajectory_meeting at the levels +-sqrt(level), the earlier of the two -- the same NaN mask, both
    residuals within bound (c); every d against rp_trajectory_separation -- NaN where sep_sq > level + 2 B, finite and no later than
    t_closest where sep_sq < level - 2 B."""
    worst = 0.0
    for family in ("random", "solved", "follower"):
        for d in (1, 2, 3):
            n, k = SHAPES[1 + d % 2]
            a, b, level, lo, hi, delay, sub = _inputs(family, d, n, k, 600 + k)
            time, _ = _con(a, b, level, lo, hi, delay)
            ok = sub[2]
            f_a = np.asarray(np.where(ok, sub[1][0], 0), dtype=np.float64)
            above = ok & (f_a > level)
            sep_sq, t_closest = sg._sep(a, b, lo, hi, delay)
            gaps = [tg._eval(x, np.where(ok, t_closest, 0.0), want=(True, False, False))[0]
                    - tg._eval(y, np.where(ok, t_closest - delay, 0.0), want=(True, False, False))[0] for x, y in zip(a, b)]
            B = sr.value_bound(a, b, gaps)
            never, surely = above & (sep_sq > level + 2 * B), above & (sep_sq < level - 2 * B)
            assert np.isnan(time[never]).all(), (family, d, "a level below the closest approach")
            assert np.isfinite(time[surely]).all() and np.all(time[surely] <= t_closest[surely]), (family, d, "a level above the closest approach")
            print("%s d = %d: f(a) above the level in %.1f %%; of those never reached %.1f %%, surely reached %.1f %%"
                  % (family, d, 100 * above.mean(), 100 * never.sum() / max(above.sum(), 1), 100 * surely.sum() / max(above.sum(), 1)))
            if d > 1:
                continue
            with np.errstate(all="ignore"):
                r = np.sqrt(np.where(level >= 0, level, np.nan))
            usable = above & ~np.isnan(r)
            r = np.where(usable, r, 1.0)
            t_p, t_m = _meet(a[0], b[0], r, lo, hi, delay), _meet(a[0], b[0], -r, lo, hi, delay)
            want = np.where(np.isnan(t_p), t_m, np.where(np.isnan(t_m), t_p, np.minimum(t_p, t_m)))
            assert np.array_equal(np.isnan(time[usable]), np.isnan(want[usable])), (family, "the NaN mask against the meeting")
            for t in (time, want):
                gone = np.isnan(t) | ~usable
                f_at, bound = _bound_c(a, b, t, delay, gone)
                worst = max(worst, float(np.where(gone, 0, np.abs(f_at - level) / bound).max()))
    print("d = 1 against rp_trajectory_meeting: residuals %.3f of bound (c)" % worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- 6. autograd
def _leaves(a, b, level, delay):
    stack = lambda v: [_t(np.stack([s[f] for s in v], axis=1)).requires_grad_() for f in range(8)]      # noqa: E731
    return stack(a), stack(b), _t(level).requires_grad_(), _t(delay).requires_grad_()


def _run(va, vb, level, lo, hi, delay):
    return rp.trajectory_contact([va[f] for f in SIX], [vb[f] for f in SIX], None, lo, hi, delay, level_sq=level)


def _by_hand(a, b, time, rate, delay, g=None, dots=None, level_dot=None, delay_dot=None):
    """The documented compositions through the evaluator's entries, elementwise arithmetic in torch on the device: reverse mode (A's and
    B's 8 d bars, level_bar, delay_bar) for g, or forward mode (time_dot) for the tangents."""
    d = len(a)
    n, k = time.shape
    missing = torch.isnan(time)
    zero = torch.zeros_like(time)
    t_a = torch.where(missing, zero, time).contiguous()
    t_b = torch.where(missing, zero, time - delay).contiguous()
    ptrs = lambda s: [_t(x) for x in s]      # noqa: E731
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=time.device)      # noqa: E731
    keep, gaps = [], []
    for x, y in zip(a, b):
        sx, sy, pa, pb = ptrs(x), ptrs(y), new(n, k), new(n, k)
        capi.trajectory_eval(0, 0, n, k, [t.data_ptr() for t in sx], t_a.data_ptr(), pa.data_ptr(), 0, 0)
        capi.trajectory_eval(0, 0, n, k, [t.data_ptr() for t in sy], t_b.data_ptr(), pb.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        keep.append((sx, sy))
        gaps.append(pa - pb)
    if g is not None:
        w = torch.where(missing, zero, g / rate)
        bars_a, bars_b, delay_bar = [], [], None
        for c, (sx, sy) in enumerate(keep):
            g_pos = ((2.0 * w) * gaps[c]).contiguous()
            neg = (-g_pos).contiguous()
            bar_a, bar_b, tau_bar = [new(n) for _ in range(8)], [new(n) for _ in range(8)], new(n, k)
            torch.cuda.synchronize()
            capi.trajectory_eval_vjp(0, 0, n, k, [t.data_ptr() for t in sx], t_a.data_ptr(), neg.data_ptr(), 0, 0, [t.data_ptr() for t in bar_a], 0)
            capi.trajectory_eval_vjp(0, 0, n, k, [t.data_ptr() for t in sy], t_b.data_ptr(), g_pos.data_ptr(), 0, 0, [t.data_ptr() for t in bar_b],
                                     tau_bar.data_ptr())
            torch.cuda.synchronize()
            bars_a.append(bar_a)
            bars_b.append(bar_b)
            delay_bar = -tau_bar if delay_bar is None else delay_bar - tau_bar
        return bars_a, bars_b, w, delay_bar
    total = level_dot
    tau_dot_b = (-delay_dot).contiguous()
    for c, (sx, sy) in enumerate(keep):
        da, db = [dots[f][:, c].contiguous() for f in range(8)], [dots[8 + f][:, c].contiguous() for f in range(8)]
        pa, pb = new(n, k), new(n, k)
        torch.cuda.synchronize()
        capi.trajectory_eval_jvp(0, 0, n, k, [t.data_ptr() for t in sx], t_a.data_ptr(), [t.data_ptr() for t in da], 0, pa.data_ptr(), 0, 0)
        capi.trajectory_eval_jvp(0, 0, n, k, [t.data_ptr() for t in sy], t_b.data_ptr(), [t.data_ptr() for t in db], tau_dot_b.data_ptr(), pb.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        total = total - (2.0 * gaps[c]) * (pa - pb)
    return torch.where(missing, torch.full_like(time, float("nan")), total / rate)


def test_autograd_reverse_forward_and_duality():
    k = 7
    for family, d in (("random", 1), ("random", 2), ("random", 3), ("solved", 2), ("follower", 2)):
        a, b, lv_np, lo_np, hi_np, dl_np, _ = _inputs(family, d, N, k, 8)
        va, vb, level, delay = _leaves(a, b, lv_np, dl_np)
        lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
        rng = np.random.default_rng(9)
        g = _t(rng.standard_normal((N, k)))
        out = _run(va, vb, level, lo, hi, delay)
        assert out.requires_grad and out.shape == (N, k)
        dev_t, dev_r = _con(a, b, lv_np, lo_np, hi_np, dl_np)
        assert _same_bits(out.detach().cpu().numpy(), dev_t), (family, d)
        leaves = va + vb + [level, delay]
        grads = torch.autograd.grad(out, leaves + [lo, hi], grad_outputs=g, retain_graph=True, allow_unused=True)
        assert all(x is None or not x.any() for x in grads[-2:]), (family, d, "lo and hi get no gradient")
        got = [x.cpu().numpy() for x in grads[:-2]]
        miss = np.isnan(dev_t)
        assert all(np.isfinite(x).all() for x in got) and all(np.all(x[miss] == 0) for x in got[16:]), (family, d)      # unreached: exactly 0
        # the composition by hand through the evaluator's entries: the same bits
        hand = _by_hand(a, b, _t(dev_t), _t(dev_r), _t(dl_np), g=g)
        flat = [torch.stack([s[f] for s in v], dim=1).cpu().numpy() for v in hand[:2] for f in range(8)] + [hand[2].cpu().numpy(), hand[3].cpu().numpy()]
        # (the bars of an (n, d) leaf are torch's sum over its d columns' gradients, each scattered into zeros: a -0.0 comes out as +0.0, so
        # the spline bars are compared as numbers, which tells every other bit apart)
        differ = [int((_bits(x) != _bits(y)).sum()) for x, y in zip(got, flat)]
        print("%s d = %d: entries whose bits differ from the composition by hand, per leaf: %s" % (family, d, differ))
        assert all(np.array_equal(x, y) for x, y in zip(got[:16], flat[:16])), (family, d, "backward against the composition by hand")
        assert all(_same_bits(x, y) for x, y in zip(got[16:], flat[16:])), (family, d, "level_bar and delay_bar against the composition by hand")
        # against the longdouble routing at the device's own times; the yardstick is the same routing on the evaluator's float64 restatement
        gn = g.cpu().numpy()
        pack = lambda r: sg._flat(r[0], r[1], r[2:])      # noqa: E731
        ref = pack(cf.derivative_ld(a, b, dl_np, dev_t, gn))
        r64 = pack(cf.derivative_ld(a, b, dl_np, dev_t, gn, vjp=tr.vjp_f64, forward=tr.forward_f64, T=np.float64))
        restated, device = float(np.max(tr.normwise(r64, ref))), float(np.max(tr.normwise(got, ref)))
        print("%s d = %d: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e"
              % (family, d, restated, device, 10 * restated))
        assert device <= 10 * restated, (family, d)
        # forward mode
        dots = [_t(rng.standard_normal((N, d))) for _ in range(16)]
        q_dot = [_t(rng.standard_normal((N, k))) for _ in range(2)]
        with fwAD.dual_level():
            dual = [fwAD.make_dual(x.detach(), t) for x, t in zip(leaves, dots + q_dot)]
            got_dot = fwAD.unpack_dual(_run(dual[:8], dual[8:16], dual[16], lo.detach(), hi.detach(), dual[17])).tangent.cpu().numpy()

        def f(*xs):
            return _run(list(xs[:8]), list(xs[8:16]), xs[16], lo.detach(), hi.detach(), xs[17])
        _, func_dot = torch.func.jvp(f, tuple(x.detach() for x in leaves), tuple(dots + q_dot))
        assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), miss), (family, d)
        hand_dot = _by_hand(a, b, _t(dev_t), _t(dev_r), _t(dl_np), dots=dots, level_dot=q_dot[0], delay_dot=q_dot[1]).cpu().numpy()
        assert _same_bits(hand_dot, got_dot), (family, d, "forward mode against the composition by hand")
        dn = [t.cpu().numpy() for t in dots + q_dot]
        split = lambda ts: [[t[:, c] for t in ts] for c in range(d)]      # noqa: E731
        zap = lambda x: np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x)      # noqa: E731
        args = (a, b, dl_np, dev_t, split(dn[:8]), split(dn[8:16]), dn[16], dn[17])
        dot_ld = zap(cf.derivative_jvp_ld(*args))
        dot64 = zap(cf.derivative_jvp_ld(*args, jvp=tr.jvp_f64, forward=tr.forward_f64, T=np.float64))
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
        (g0,) = torch.autograd.grad((torch.nan_to_num(_run(va, vb, level, lo, hi, delay)) ** 2).sum(), va[1], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        # reverse mode against central differences of the device op, on the yardstick mask: 1e-6 normwise
        keep = ~miss & cf.difference_is_a_yardstick(a, b, lv_np, dl_np, dev_t)
        gk = np.where(keep, gn, 0.0)
        gk_t = _t(gk)
        analytic = [x.cpu().numpy() for x in torch.autograd.grad(out, leaves, grad_outputs=gk_t, retain_graph=True)]
        steps_a, steps_b, level_step, delay_step = cf.difference_steps(a, b, lv_np, dl_np)
        stable = np.ones(N, dtype=bool)

        def F(sa, sb, lv, dl):
            nonlocal stable
            t = _con(sa, sb, lv, lo_np, hi_np, dl, want_rate=False)[0]
            stable &= ~(np.isnan(t) & keep).any(axis=1)
            return np.where(keep, gk * t, 0.0)

        fd = []
        for which in range(2):
            for f in range(8):
                cols = []
                for x in range(d):
                    h = (steps_a, steps_b)[which][x][f]
                    up, dn_ = ([[v.copy() for v in s] for s in (a, b)[which]] for _ in range(2))
                    up[x][f], dn_[x][f] = up[x][f] + h, dn_[x][f] - h
                    diff = F(up, b, lv_np, dl_np) - F(dn_, b, lv_np, dl_np) if which == 0 else F(a, up, lv_np, dl_np) - F(a, dn_, lv_np, dl_np)
                    cols.append(diff.sum(axis=1) / (up[x][f] - dn_[x][f]))
                fd.append(np.stack(cols, axis=1))
        up, dn_ = lv_np + level_step, lv_np - level_step
        fd.append((F(a, b, up, dl_np) - F(a, b, dn_, dl_np)) / (up - dn_))
        up, dn_ = dl_np + delay_step, dl_np - delay_step
        fd.append((F(a, b, lv_np, up) - F(a, b, lv_np, dn_)) / (up - dn_))
        some = keep.any(axis=1) & stable
        err = float(np.max(tr.normwise([x[some].reshape(some.sum(), -1) for x in analytic], [x[some].reshape(some.sum(), -1) for x in fd])))
        print("%s d = %d: the yardstick mask keeps %.1f %% of the reached queries, %.1f %% of the problems stay; reverse mode against central "
              "differences of the device op %.2e normwise" % (family, d, 100 * keep.sum() / max((~miss).sum(), 1), 100 * some.mean(), err))
        assert keep.sum() >= 0.5 * (~miss).sum() and some.mean() > 0.5 and err < 1e-6, (family, d, err)
        if (family, d) != ("random", 2):
            continue
        # the radius: the level is radius * radius formed in torch, so radius.grad is 2 radius level_bar; a (k,) radius is every problem's
        radius = torch.sqrt(level.detach().clamp(min=0.0)).requires_grad_()
        sq = (radius.detach() * radius.detach()).requires_grad_()
        six = lambda v: [v[f].detach() for f in SIX]      # noqa: E731
        t_r = rp.trajectory_contact(six(va), six(vb), radius, lo.detach(), hi.detach(), delay.detach())
        t_s = rp.trajectory_contact(six(va), six(vb), None, lo.detach(), hi.detach(), delay.detach(), level_sq=sq)
        assert _same_bits(t_r.detach().cpu().numpy(), t_s.detach().cpu().numpy())
        (r_bar,), (s_bar,) = torch.autograd.grad(t_r, radius, grad_outputs=g), torch.autograd.grad(t_s, sq, grad_outputs=g)
        assert torch.isfinite(r_bar).all() and torch.equal(r_bar, 2.0 * radius.detach() * s_bar), "radius.grad == 2 radius level_bar"
        row = torch.full((k,), 30.0, dtype=torch.float64, device=radius.device, requires_grad=True)
        t_row = rp.trajectory_contact(six(va), six(vb), row, lo.detach(), hi.detach(), delay.detach())
        assert _same_bits(t_row.detach().cpu().numpy(), _con(a, b, np.full((N, k), 900.0), lo_np, hi_np, dl_np)[0])
        (row_bar,) = torch.autograd.grad(torch.nan_to_num(t_row).sum(), row)
        assert row_bar.shape == (k,) and torch.isfinite(row_bar).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. through the solves
def test_the_pipeline_against_central_differences():
    """min_time_contact (d = 2, synchronised, gap 1e-13) on 300 golden problems per axis against themselves 25 lower on both axes, delays
    U(0.02, 0.3) T, levels from contact_ref.levels on the device's own solutions, against central differences of the whole device pipeline
    in pos1 of each vehicle and axis (h = 1e-4), on converged finite queries that pass the yardstick mask: section 15's pipeline bound,
    median < 1e-5 and 95 % < 1e-3, in more than half of the problems."""
    n, k, d = N, 8, 2
    pos = gg._golden_positions(d * n).reshape(d, n, 3)
    xa = [_t(pos[:, :, c].T).requires_grad_() for c in range(3)]
    xb = [_t(pos[:, :, c].T - 25.0).requires_grad_() for c in range(3)]

    def pipeline(pa, pb, level, lo, hi, delay):
        return rp.min_time_contact(pa, pb, None, lo, hi, delay, level_sq=level, gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(xa, xb, _t(np.full((n, 1), 625.0)), None, None, None)
    assert len(first) == 3 and len(first[1]) == 5 and len(first[2]) == 5 and all(t.shape == (n, d) for t in first[1] + first[2])
    assert first[0].shape == (n, 1)
    conv = np.ones(n, dtype=bool)
    vehicles = []
    for x, sol in zip((xa, xb), first[1:]):
        s = [t.cpu().numpy() for t in sol[:3]]
        conv &= (np.isfinite(np.stack(s, 2)).all(2) & (s[1] > 0) & (s[2] > 0) & ((sol[4] & capi.ST_CONVERGED) != 0).cpu().numpy()).all(axis=1)
        stretched, _ = rp.synchronize_axes([t.detach() for t in x] + [t for t in sol[:3]])
        st = [t.cpu().numpy() for t in stretched]
        z = np.zeros(n)
        vehicles.append([[v for v in (st[0][:, c], st[1][:, c], st[2][:, c], z, z, st[3][:, c], st[4][:, c], st[5][:, c])] for c in range(d)])
    print("%d of %d pairs converged" % (int(conv.sum()), n))
    assert conv.mean() > 0.95
    a, b = ([[np.where(conv, v, 1.0) for v in s] for s in vehicle] for vehicle in vehicles)
    dl_np = sr.delays(a, b, k, 23, follow=True)      # fixed times and levels: the queries do not move with the solutions
    lo_np, hi_np = sr.windows(a, b, dl_np, 24)
    lv_np = cf.levels(a, b, lo_np, hi_np, dl_np, 26)[0]
    level, lo, hi, delay = _t(lv_np), _t(lo_np), _t(hi_np), _t(dl_np)
    out = pipeline(xa, xb, level, lo, hi, delay)
    t_np = out[0].detach().cpu().numpy()
    finite = conv[:, None] & np.isfinite(t_np)
    keep_np = finite & cf.difference_is_a_yardstick(a, b, lv_np, dl_np, np.where(finite, t_np, np.nan))
    keep = _t(keep_np).bool()
    wt = _t(np.random.default_rng(25).uniform(0.5, 1.5, (n, k)))
    h = 1e-4
    rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
    grads = torch.autograd.grad(rows(out[0]).sum(), [xa[1], xb[1]])
    some = _t(keep_np.any(axis=1)).bool()
    print("%.0f %% of the levels reached; %.0f %% of the converged, finite queries pass the yardstick mask, in %.0f %% of the problems"
          % (100 * finite.mean(), 100 * keep_np.sum() / finite.sum(), 100 * float(some.float().mean())))
    with torch.no_grad():
        for which, vehicle in enumerate("ab"):
            for c in range(d):
                step = torch.zeros_like(xa[1])
                step[:, c] = h
                up, dn = [list(xa), list(xb)], [list(xa), list(xb)]
                up[which][1], dn[which][1] = up[which][1] + step, dn[which][1] - step
                fd = (rows(pipeline(up[0], up[1], level, lo, hi, delay)[0]) - rows(pipeline(dn[0], dn[1], level, lo, hi, delay)[0])) / (2 * h)
                ok = some & torch.isfinite(fd) & torch.isfinite(grads[which][:, c])
                rel = ((grads[which][:, c] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]
                print("  d t_contact / d pos1 of %s, axis %d, against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% of the problems)"
                      % (vehicle, c, rel.median(), rel.quantile(0.95), 100 * float(ok.float().mean())))
                assert float(ok.float().mean()) > 0.5 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, (vehicle, c)
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
