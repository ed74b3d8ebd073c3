"""The cases of tests/test_gpu_extrema.py, each run in a fresh process (`python tests/extrema_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound is
what it is: DESIGN.md section 15."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import crossing_ref as cr  # noqa: E402
import extrema_ref as xr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV, BIG = tg.DEV, tg.BIG
KS = (1, 2, 7, 8)      # odd k and odd totals (BIG is odd) take the unpaired path of stream_pairs
LD = np.longdouble
FAMILIES = ("solved", "random", "rest", "knot")
NAMES = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")
ALL = (True,) * 4
_t, _bits, _same_bits, _head, Out = tg._t, tg._bits, tg._same_bits, tg._head, tg.Out


def _family(name):
    """One spline of BIG problems: trajectory_gpu_cases' device-solved ones (kappa = 0.1), random unsolved ones, rest-to-rest random ones;
    `knot` is extrema_ref.knot_cases' eight."""
    if name == "solved":
        return tg._families()["solved"]
    if name == "knot":
        return xr.knot_cases()[0]
    return tr.random_states(BIG, 5) if name == "random" else cr.rest_to_rest(BIG, 6)


def _windows(name, sp, k, seed):
    if name == "knot":      # its own window in every column
        _, lo, hi, _ = xr.knot_cases()
        return np.repeat(lo, k, axis=1), np.repeat(hi, k, axis=1)
    return xr.windows(sp, k, seed)


def _ext(sp, lo, hi, k=None, values=ALL, times=ALL, zero_vel=False):
    """The stateless entry: (four values, four times), None where not asked for.  lo / hi of None go in as NULL."""
    n = len(sp[0])
    k = k if k is not None else (lo if lo is not None else hi).shape[1]
    ts = [_t(a) for a in sp]
    tl, th = (_t(a) if a is not None else None for a in (lo, hi))
    outs = [Out(n, k) if w else None for w in tuple(values) + tuple(times)]
    addr = [t.data_ptr() for t in ts]
    if zero_vel:
        addr[3] = addr[4] = 0
    ptr = [o.ptr if o else 0 for o in outs]
    capi.trajectory_extrema(0, 0, n, k, addr, tl.data_ptr() if tl is not None else 0, th.data_ptr() if th is not None else 0, ptr[:4], ptr[4:])
    torch.cuda.synchronize()
    got = [o.get() if o else None for o in outs]
    return got[:4], got[4:]


def _all_same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    sp = _family(family)
    n = len(sp[0])
    sc, T = tr.scales(sp), (sp[6] + sp[7])[:, None]
    worst = {"value, of its bound": 0.0, "time off ties, of T": 0.0, "the float64 restatement's time, of T": 0.0}
    for k in KS:
        lo, hi = _windows(family, sp, k, 300 + k)
        want_v, want_t = xr.extrema_ld(sp, lo, hi)
        v64, t64 = xr.extrema_f64(sp, lo, hi)
        gap = xr.runner_up_gap(sp, lo, hi)
        got_v, got_t = _ext(sp, lo, hi)
        for j, name in enumerate(xr.NAMES):
            missing = np.isnan(want_v[j])
            assert np.array_equal(np.isnan(got_v[j]), missing) and np.array_equal(np.isnan(got_t[j]), missing), (family, k, name, "the NaN mask")
            err = np.where(missing, 0, np.abs(got_v[j] - want_v[j]) / (1e-13 * sc[0 if j < 2 else 1]))
            worst["value, of its bound"] = max(worst["value, of its bound"], float(err.max()))
            clear = ~missing & (gap[j] >= 1e-9)
            worst["time off ties, of T"] = max(worst["time off ties, of T"], float(np.where(clear, np.abs(got_t[j] - want_t[j]) / T, 0).max()))
            worst["the float64 restatement's time, of T"] = max(worst["the float64 restatement's time, of T"],
                                                                float(np.where(clear, np.abs(t64[j] - want_t[j]) / T, 0).max()))
        if family == "knot":
            for i, kind in enumerate(xr.knot_cases()[3]):
                j = xr.NAMES.index(kind)
                assert np.all(got_v[j][i] == (sp[1][i] if j < 2 else sp[5][i])) and np.all(got_t[j][i] == sp[6][i]), (i, kind)
        # a NULL window end is the infinite one, bit for bit (column 0 has both)
        inf = np.full(lo.shape, np.inf)
        assert _all_same(_ext(sp, None, hi), _ext(sp, -inf, hi)) and _all_same(_ext(sp, lo, None), _ext(sp, lo, inf)), (family, k)
        assert _all_same(_ext(sp, None, None, k=k), _ext(sp, -inf, inf)), (family, k)
        if k == 7:
            # every output alone, and every output alone left out: the others' bits do not change, and nothing else is written
            full = got_v + got_t
            for f in range(8):
                for alone in (True, False):
                    want = [(g == f) == alone for g in range(8)]
                    some = _ext(sp, lo, hi, values=want[:4], times=want[4:])
                    for g, x in enumerate(some[0] + some[1]):
                        assert (x is None) == (not want[g]) and (x is None or _same_bits(x, full[g])), (family, f, alone, g)
    print("%s (%d problems) x %s: %s" % (family, n, KS, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["value, of its bound"] <= 1.0
    # times off ties: ten times what the float64 restatement of the rule holds on the same inputs (section 12's margin)
    assert worst["time off ties, of T"] <= 10 * worst["the float64 restatement's time, of T"]
    if family == "knot":
        return
    # the NaN rule: a duration of 0, -1, inf, NaN poisons its problem and no other; a NaN window end its own query and no other
    m, k = 257, 7
    sp = [a.copy() for a in _head(sp, m)]
    lo, hi = xr.windows(sp, k, 1)
    clean = _ext(sp, lo, hi)
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    bad = np.zeros((m, k), dtype=bool)
    bad[[3, 64, 130, 256]] = True
    bad[10, 0] = bad[200, 4] = bad[11, 3] = True
    got = _ext(sp, lo, hi)
    for x, ref in zip(got[0] + got[1], clean[0] + clean[1]):
        assert np.array_equal(np.isnan(x), bad | np.isnan(ref)), family
        assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad])), family
    if family == "rest":      # NULL end velocities are zeros
        assert _all_same(_ext(_head(_family(family), 65), lo[:65], hi[:65], zero_vel=True), _ext(_head(_family(family), 65), lo[:65], hi[:65]))


# ---------------------------------------------------------------- 2. the invariant
def test_every_value_is_the_evaluators_at_the_returned_time():
    for family in FAMILIES:
        sp = _family(family)
        for k in KS:
            lo, hi = _windows(family, sp, k, 400 + k)
            values, times = _ext(sp, lo, hi)
            for j in range(4):
                missing = np.isnan(times[j])
                out = tg._eval(sp, times[j], want=(j < 2, j >= 2, False))[0 if j < 2 else 1]
                assert np.array_equal(np.isnan(values[j]), missing) and np.isnan(out[missing]).all(), (family, k, xr.NAMES[j])
                assert np.array_equal(_bits(out[~missing]), _bits(values[j][~missing])), (family, k, xr.NAMES[j])
    print("every value is rp_trajectory_eval's at the returned time, bit for bit")


# ---------------------------------------------------------------- 3. the batch entry
def test_batch_entry_equals_the_stateless_one():
    orc = Oracle()
    n = BIG
    for variant, dtype in ((rp.VARIANT_F3, rp.DTYPE_F64), (rp.VARIANT_F4, rp.DTYPE_F64), (rp.VARIANT_F4, rp.DTYPE_F32_STATE)):
        for vel in (True, False):
            args = tg._inputs(orc, 0.1, n)
            with rp.Batch(n, variant, dtype) as b:
                ts = [_t(a) for a in args]
                if vel:
                    b.set_problems_vel_device(*[t.data_ptr() for t in ts])
                else:
                    b.set_problems_device(*[t.data_ptr() for t in ts[:3]])
                b.solve(1e-8, 200, 0)
                assert not np.array_equal(b.slot_map(), np.arange(n)), "the batch kept problem order: nothing to gather"
                sp = tr.spline_of_state(b.get_state(), variant)
                for k in KS:
                    lo, hi = xr.windows(sp, k, 12 + k)
                    tl, th = _t(lo), _t(hi)
                    outs = [Out(n, k) for _ in range(8)]
                    b.extrema_device(tl.data_ptr(), th.data_ptr(), k, [o.ptr for o in outs[:4]], [o.ptr for o in outs[4:]])
                    b.sync()
                    got = [o.get() for o in outs]
                    want = _ext(sp, lo, hi)
                    assert all(_same_bits(x, y) for x, y in zip(got, want[0] + want[1])), (variant, dtype, vel, k)
                    only = Out(n, k)
                    b.extrema_device(0, 0, k, [0, 0, 0, only.ptr], None)      # the whole spline's top speed upward, nothing else
                    b.sync()
                    assert _same_bits(only.get(), _ext(sp, None, None, k=k)[0][3])
                finite = float((~np.isnan(got[0])).mean())
                print("variant %d dtype %d vel %s: the batch entry's bits are the stateless entry's; %.1f %% of the windows not empty" % (variant, dtype, vel, 100 * finite))
                assert finite > 0.9


# ---------------------------------------------------------------- 4. reproducibility
def test_bits_depend_on_the_problem_and_its_window_only():
    for family in ("solved", "random", "rest"):
        sp = _family(family)
        for k in KS:
            lo, hi = xr.windows(sp, k, 500 + k)
            first = _ext(sp, lo, hi)
            assert _all_same(first, _ext(sp, lo, hi)), "differs from run to run"
            for n in (1, 129, 4096):
                assert _all_same(_ext(_head(sp, n), lo[:n], hi[:n]), ([x[:n] for x in first[0]], [x[:n] for x in first[1]])), (family, n, k)
            roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
            moved = _ext([roll(a) for a in sp], roll(lo), roll(hi))
            for a, b in zip(moved[0] + moved[1], first[0] + first[1]):
                assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (family, k)
    # more trips than the grid's cap: 300,001 problems of one window each are 2,344 trips of 128 for 2,048 blocks
    n = 300001
    sp = tr.random_states(n, 77)
    lo, hi = (x[:, 2:3].copy() for x in xr.windows(sp, 3, 78))
    got_v, got_t = _ext(sp, lo, hi)
    v64, t64 = xr.extrema_f64(sp, lo, hi)
    sc = tr.scales(sp)
    worst = 0.0
    for j in range(4):
        missing = np.isnan(v64[j])
        assert np.array_equal(np.isnan(got_v[j]), missing) and np.array_equal(np.isnan(got_t[j]), missing), xr.NAMES[j]
        worst = max(worst, float(np.where(missing, 0, np.abs(got_v[j] - v64[j]) / sc[0 if j < 2 else 1]).max()))
    print("%d problems x 1 window: %.2f %% empty, values within %.2e of the scale of the float64 restatement" % (n, 100 * missing.mean(), worst))
    assert 0.002 < missing.mean() < 0.03 and worst <= 1e-13
    # two windows each (a trip is still 128 problems): the rows at the start, where the blocks begin their second trip and at the end are
    # those of a batch of their own
    lo, hi = xr.windows(sp, 2, 79)
    tg.rows_equal_their_own_batch(("extrema", 2), lambda s, a, b: (lambda r: r[0] + r[1])(_ext(s, a, b)), sp, lo, hi)


# ---------------------------------------------------------------- 5. autograd
def _by_hand(ins, lo, hi, outs, g):
    """The documented reverse composition on the device: the classes by equality, one rp_trajectory_eval_vjp launch at the four time arrays
    side by side, tau_bar routed.  Returns the ten gradients as numpy arrays, and (the evaluator's own eight bars, tau_bar)."""
    n, k = outs[0].shape
    time = torch.cat([o.detach() for o in outs[4:]], dim=1)
    missing = torch.isnan(torch.cat([o.detach() for o in outs[:4]], dim=1)) | torch.isnan(time)
    t0 = torch.where(missing, torch.zeros_like(time), time).contiguous()
    d0, T = ins["duration0"].detach().unsqueeze(1), (ins["duration0"] + ins["duration1"]).detach().unsqueeze(1)
    is_lo = (t0 == lo.detach().repeat(1, 4)) & ~missing
    is_hi = (t0 == hi.detach().repeat(1, 4)) & ~missing & ~is_lo
    is_end = (t0 == T) & ~missing & ~is_lo & ~is_hi
    is_knot = (t0 == d0) & ~missing & ~is_lo & ~is_hi & ~is_end
    zero = torch.zeros((n, k), dtype=torch.float64, device=DEV)
    g_pos = torch.where(missing, torch.zeros_like(t0), torch.cat([g[0], g[1], zero, zero], dim=1)).contiguous()
    g_vel = torch.where(missing, torch.zeros_like(t0), torch.cat([zero, zero, g[2], g[3]], dim=1)).contiguous()
    bars, tau_bar = [Out(n) for _ in range(8)], Out(n, 4 * k)
    capi.trajectory_eval_vjp(0, 0, n, 4 * k, [ins[nm].data_ptr() for nm in NAMES], t0.data_ptr(), g_pos.data_ptr(), g_vel.data_ptr(), 0,
                             [o.ptr for o in bars], tau_bar.ptr)
    torch.cuda.synchronize()
    raw = [_t(o.get()) for o in bars]
    tb = _t(tau_bar.get())
    routed = lambda mask: torch.where(mask, tb, torch.zeros_like(tb))      # noqa: E731
    fold = lambda x: x.reshape(n, 4, k).sum(dim=1)      # noqa: E731
    end = routed(is_end).sum(dim=1)
    hand = list(raw)
    hand[6] = raw[6] + (end + routed(is_knot).sum(dim=1))
    hand[7] = raw[7] + end
    hand += [fold(routed(is_lo)), fold(routed(is_hi))]
    masks = (t0, missing, is_lo, is_hi, is_end, is_knot)
    return [x.cpu().numpy() for x in hand], ([x.cpu().numpy() for x in raw], tb.cpu().numpy()), masks


def test_autograd_reverse_forward_and_duality():
    n, k = BIG, 7
    for family in ("solved", "random", "rest"):
        sp = _family(family)
        lo_np, hi_np = xr.windows(sp, k, 8)
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
        lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
        rng = np.random.default_rng(9)
        g = [_t(rng.standard_normal((n, k))) for _ in range(4)]

        def run(v, a, b):
            return rp.trajectory_extrema(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], a, b, vel0=v["vel0"], vel2=v["vel2"])

        outs = run(ins, lo, hi)
        assert len(outs) == 8 and not any(o.requires_grad for o in outs[4:]) and all(o.requires_grad for o in outs[:4])
        dev_v, dev_t = _ext(sp, lo_np, hi_np)
        assert all(_same_bits(o.detach().cpu().numpy(), x) for o, x in zip(outs, dev_v + dev_t)), family
        leaves = [ins[nm] for nm in NAMES] + [lo, hi]
        grads = torch.autograd.grad(outs[:4], leaves, grad_outputs=g, retain_graph=True)
        got = [x.cpu().numpy() for x in grads]
        hand, _, (t0, missing, is_lo, is_hi, is_end, is_knot) = _by_hand(ins, lo, hi, outs, g)
        assert all(_same_bits(a, b) for a, b in zip(got, hand)), family
        miss = missing.cpu().numpy()
        assert all(np.isfinite(x).all() for x in got) and np.all(got[8][miss[:, :k]] == 0) and np.all(got[9][miss[:, :k]] == 0), family
        shares = [float(m.float().mean()) for m in (is_lo, is_hi, is_end, is_knot)]
        print("%s: classes of the returned times: LO %.3f HI %.3f END %.3f KNOT %.3f, no value %.3f" % ((family,) + tuple(shares) + (float(miss.mean()),)))
        assert min(shares[:3]) > 0.01 and (family != "solved" or shares[3] > 0.01)
        # forward mode by hand: one rp_trajectory_eval_jvp launch with tau_dot routed the same way
        dots = [_t(d) for d in tg._tangents(n, k, 10)[0]]
        lo_dot, hi_dot = _t(rng.standard_normal((n, k))), _t(rng.standard_normal((n, k)))
        col = lambda t: t.unsqueeze(1).expand(n, 4 * k)      # noqa: E731
        tau_dot = torch.zeros_like(t0)
        tau_dot = torch.where(is_lo, lo_dot.repeat(1, 4), tau_dot)
        tau_dot = torch.where(is_hi, hi_dot.repeat(1, 4), tau_dot)
        tau_dot = torch.where(is_end | is_knot, col(dots[6]), tau_dot)
        tau_dot = torch.where(is_end, tau_dot + col(dots[7]), tau_dot).contiguous()
        pd, vd = Out(n, 4 * k), Out(n, 4 * k)
        capi.trajectory_eval_jvp(0, 0, n, 4 * k, [ins[nm].data_ptr() for nm in NAMES], t0.data_ptr(), [d.data_ptr() for d in dots], tau_dot.data_ptr(),
                                 pd.ptr, vd.ptr, 0)
        torch.cuda.synchronize()
        pd, vd = np.where(miss, np.nan, pd.get()), np.where(miss, np.nan, vd.get())
        want_dot = [pd[:, :k], pd[:, k:2 * k], vd[:, 2 * k:3 * k], vd[:, 3 * k:]]
        with fwAD.dual_level():
            dual = {nm: fwAD.make_dual(ins[nm].detach(), d) for nm, d in zip(NAMES, dots)}
            douts = run(dual, fwAD.make_dual(lo.detach(), lo_dot), fwAD.make_dual(hi.detach(), hi_dot))
            got_dot = [fwAD.unpack_dual(o).tangent.cpu().numpy() for o in douts[:4]]
            assert all(fwAD.unpack_dual(o).tangent is None for o in douts[4:])
        assert all(_same_bits(a, b) for a, b in zip(got_dot, want_dot)), family

        def f(*xs):
            return run(dict(zip(NAMES, xs[:8])), xs[8], xs[9])[:4]
        _, func_dot = torch.func.jvp(f, tuple(x.detach() for x in leaves), tuple(dots) + (lo_dot, hi_dot))
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(func_dot, want_dot)), family
        # against the longdouble routing at the device's own times; the yardstick is the same routing on the evaluator's float64 restatement
        gn = [x.cpu().numpy() for x in g]
        ref = xr.derivative_ld(sp, lo_np, hi_np, dev_t, dev_v, gn)
        ref = list(ref[0]) + [ref[1], ref[2]]
        r64 = xr.derivative_ld(sp, lo_np, hi_np, dev_t, dev_v, gn, vjp=tr.vjp_f64)
        r64 = list(r64[0]) + [r64[1], r64[2]]
        restated, device = float(np.max(tr.normwise(r64, ref))), float(np.max(tr.normwise(got, ref)))
        print("%s: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        dn = [d.cpu().numpy() for d in dots]
        ldn, hdn = lo_dot.cpu().numpy(), hi_dot.cpu().numpy()
        zap = lambda xs: [np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x) for x in xs]      # noqa: E731
        dot_ld = zap(xr.derivative_jvp_ld(sp, lo_np, hi_np, dev_t, dev_v, dn, ldn, hdn))
        dot64 = zap(xr.derivative_jvp_ld(sp, lo_np, hi_np, dev_t, dev_v, dn, ldn, hdn, jvp=tr.jvp_f64))
        restated, device = float(np.max(tr.normwise(dot64, dot_ld))), float(np.max(tr.normwise(zap(got_dot), dot_ld)))
        print("%s: forward mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # duality between the two modes: <g, J u> = <J^T g, u>
        left_terms = [np.where(np.isnan(d), 0, x.astype(LD) * d) for x, d in zip(gn, got_dot)]
        right_terms = [x.astype(LD) * d for x, d in zip(got[:8], dn)] + [got[8].astype(LD) * ldn, got[9].astype(LD) * hdn]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        size = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, family
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(run(ins, lo, hi)[3]) ** 2).sum(), ins["vel1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        if family != "random":
            continue
        # column 0, the whole spline: where pos_max is at the END its gradient reaches pos2, and what the evaluator puts on the durations at
        # a fixed time is cancelled by the routed tau_bar to 1e-12 of the largest term
        at_end = (dev_t[1][:, 0] == sp[6] + sp[7])
        assert at_end.mean() > 0.05
        one = torch.zeros((n, k), dtype=torch.float64, device=DEV)
        one[:, 0] = 1.0
        zeros = torch.zeros_like(one)
        total = [x.cpu().numpy() for x in torch.autograd.grad(outs[1], leaves, grad_outputs=one, retain_graph=True)]
        _, (raw, tb), _ = _by_hand(ins, lo, hi, outs, [zeros, one, zeros, zeros])
        tb = tb[:, k]      # pos_max's column 0 in the side-by-side layout
        largest = np.maximum(np.maximum(np.abs(raw[6]), np.abs(raw[7])), np.maximum(np.abs(tb), 1.0))
        left_over = np.maximum(np.abs(total[6]), np.abs(total[7])) / largest
        print("pos_max at the END (%.0f %% of the problems): d / d pos2 in [%.17g, %.17g], %.2e of the largest term left on the durations (that term up to %.3g)"
              % (100 * at_end.mean(), total[2][at_end].min(), total[2][at_end].max(), left_over[at_end].max(), largest[at_end].max()))
        assert np.all(np.abs(total[2][at_end] - 1.0) <= 1e-12) and left_over[at_end].max() <= 1e-12
        # a (k,) window is every problem's; both None: k = 1, the whole spline; vel0 / vel2 of None are zeros
        z = np.zeros(n)
        flat = [sp[0], sp[1], sp[2], z, z, sp[5], sp[6], sp[7]]
        six = [ins[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        row_lo, row_hi = _t(np.array([0.1, 0.2, 0.3])).requires_grad_(), _t(np.array([0.5, 0.25, 9.0]))
        o = rp.trajectory_extrema(*six, row_lo, row_hi)
        want = _ext(flat, np.repeat([[0.1, 0.2, 0.3]], n, axis=0), np.repeat([[0.5, 0.25, 9.0]], n, axis=0))
        assert all(_same_bits(a.detach().cpu().numpy(), b) for a, b in zip(o, want[0] + want[1]))
        (g_row,) = torch.autograd.grad(torch.nan_to_num(o[0]).sum(), row_lo)
        assert g_row.shape == (3,)
        whole = rp.trajectory_extrema(*six)
        want = _ext(flat, None, None, k=1)
        assert whole[0].shape == (n, 1) and all(_same_bits(a.cpu().numpy(), b) for a, b in zip(whole, want[0] + want[1]))
        only_hi = rp.trajectory_extrema(*six, None, row_hi)
        want = _ext(flat, None, np.repeat([[0.5, 0.25, 9.0]], n, axis=0))
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(only_hi, want[0] + want[1]))
    # the knot family: a kink extreme of vel at the knot moves as vel1 and not with duration0
    sp, lo_np, hi_np, kinds = xr.knot_cases()
    ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
    outs = rp.trajectory_extrema(ins["pos0"], ins["pos1"], ins["pos2"], ins["vel1"], ins["duration0"], ins["duration1"], _t(lo_np), _t(hi_np),
                                 vel0=ins["vel0"], vel2=ins["vel2"])
    for j, name in enumerate(xr.NAMES):
        rows = np.array([kd == name for kd in kinds])
        gr = [x.cpu().numpy()[rows] for x in torch.autograd.grad(outs[j].sum(), [ins[nm] for nm in NAMES], retain_graph=True)]
        assert np.all(outs[4 + j].cpu().numpy()[rows, 0] == sp[6][rows]), name
        unit = 1 if j < 2 else 5      # pos1 for the position cases, vel1 for the velocity cases
        print("knot cases, %s: d / d %s %s, d / d duration0 %s" % (name, NAMES[unit], gr[unit], gr[6]))
        assert np.all(np.abs(gr[unit] - 1.0) <= 1e-12) and np.all(np.abs(gr[6]) <= 1e-12), name
        assert all(np.all(np.abs(gr[f]) <= 1e-12) for f in range(8) if f not in (unit, 6)), name
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. through the solve
def test_the_pipeline_against_central_differences():
    orc = Oracle()
    n, k = 4096, 8
    args = tg._inputs(orc, 0.1, n)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}

    def pipeline(v, a, b):
        return rp.min_time_extrema(v["pos0"], v["pos1"], v["pos2"], a, b, vel0=v["vel0"], vel2=v["vel2"], gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(x, None, None)
    sol = [t.cpu().numpy() for t in first[8:11]]
    live = np.isfinite(np.stack(sol, 1)).all(1) & (sol[1] > 0) & (sol[2] > 0)
    sp = [np.where(live, a, 1.0) for a in tuple(args) + tuple(sol)]
    lo_np, hi_np = xr.windows(sp, k, 23)      # fixed times: the windows do not move with the solution
    lo, hi = _t(lo_np), _t(hi_np)
    out = pipeline(x, lo, hi)
    assert len(out) == 13
    status = out[12]
    gap = xr.runner_up_gap(sp, lo_np, hi_np)
    rng = np.random.default_rng(24)
    wt = _t(rng.uniform(0.5, 1.5, (n, k)))
    conv = ((status & capi.ST_CONVERGED) != 0).cpu().numpy() & live
    print("%d of %d problems converged" % (int(conv.sum()), n))
    assert conv.mean() > 0.95
    h = 1e-4
    moved = {}
    with torch.no_grad():
        for nm in names:
            up, dn = dict(x), dict(x)
            up[nm], dn[nm] = x[nm] + h, x[nm] - h
            moved[nm] = (pipeline(up, lo, hi)[:4], pipeline(dn, lo, hi)[:4])
    for j, name in enumerate(xr.NAMES):
        finite = conv[:, None] & np.isfinite(out[j].detach().cpu().numpy())
        keep_np = finite & (gap[j] >= 1e-2)
        keep_np[:, 1] = False      # hi sits on the solution's knot: a kink in every input
        share = keep_np.sum() / finite[:, [0] + list(range(2, k))].sum()
        keep = _t(keep_np).bool()
        rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
        grads = torch.autograd.grad(rows(out[j]).sum(), [x[nm] for nm in names], retain_graph=True)
        print("%s: %.0f %% of the converged, finite queries lead by 1e-2 of the scale" % (name, 100 * share))
        assert share > 0.5, name
        some = _t(keep_np.any(axis=1)).bool()
        for i, nm in enumerate(names):
            fd = (rows(moved[nm][0][j]) - rows(moved[nm][1][j])) / (2 * h)
            ok = some & torch.isfinite(fd) & torch.isfinite(grads[i])
            rel = ((grads[i] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]
            print("  d %s / d %-5s against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% of the problems)"
                  % (name, nm, rel.median(), rel.quantile(0.95), 100 * float(ok.float().mean())))
            assert float(ok.float().mean()) > 0.5 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, (name, nm)
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
