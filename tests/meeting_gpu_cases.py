"""The cases of tests/test_gpu_meeting.py, each run in a fresh process (`python tests/meeting_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's and tests/gap_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is
checked, and why each bound is what it is: DESIGN.md section 22."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_gpu_cases as gg  # noqa: E402
import gap_ref as gr  # noqa: E402
import meeting_ref as mr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

N, SHAPES, NAMES, LD, EPS = gg.N, gg.SHAPES, gg.NAMES, np.longdouble, mr.EPS
FAMILIES = ("random", "solved", "follower")
_t, _bits, _same_bits, Out = tg._t, tg._bits, tg._same_bits, tg.Out


def _queries(family, a, b, delays, k, seed):
    """(level, lo, hi, delay, reached): section 18's delays and windows, meeting_ref's levels on these very splines."""
    lo, hi, delay = gg._queries(family, a, b, delays, k, seed)
    level, reached, _ = mr.levels(a, b, lo, hi, delay, seed + 2)
    return level, lo, hi, delay, reached


def _meeting(a, b, level, lo, hi, delay, k=None, relvel=True, zero_vel=False):
    """The stateless entry: (time, relvel or None).  level / lo / hi / delay of None go in as NULL."""
    n = len(a[0])
    k = k if k is not None else next(x for x in (level, lo, hi, delay) if x is not None).shape[1]
    ta, tb = [_t(x) for x in a], [_t(x) for x in b]
    qs = [_t(x) if x is not None else None for x in (level, lo, hi, delay)]
    time, vel = Out(n, k), Out(n, k) if relvel else None
    addr_a, addr_b = [t.data_ptr() for t in ta], [t.data_ptr() for t in tb]
    if zero_vel:
        addr_a[3] = addr_a[4] = addr_b[3] = addr_b[4] = 0
    capi.trajectory_meeting(0, 0, n, k, addr_a, addr_b, *[t.data_ptr() if t is not None else 0 for t in qs], time.ptr, vel.ptr if vel else 0)
    torch.cuda.synchronize()
    return time.get(), vel.get() if vel else None


def _both_same(x, y):
    return _same_bits(x[0], y[0]) and _same_bits(x[1], y[1])


def _bound_c(a, b, level, delay, time, residual):
    """residual / ((c) = 2e-13 scale + 4 eps Tmax |relvel|) at the times given (NaN: 0), relvel the longdouble one there; and that relvel"""
    ok = ~np.isnan(time)
    at = np.where(ok, time, 0.0).astype(LD)
    d_ld, v_ld = mr.gap_ld(a, b, at, np.where(ok, delay, 0.0))
    res = np.abs(d_ld - level) if residual is None else np.abs(residual)
    return np.where(ok, res / (2e-13 * gr.scale(a, b) + 4 * EPS * mr.tmax(a, b, delay) * np.abs(v_ld)), 0), v_ld


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    """The CPU table's bounds: NaN mask identical, each time inside the definition's sub-piece to 4 eps Tmax, the longdouble residual within
    (c), relvel within 2e-13 max(X / tmin, 1) of the longdouble closing velocity at the device's time; the hand-made cases' bits."""
    if family == "hand":
        a, b, level, lo, hi, delay, want = mr.hand_made()
        for k in (1, 7, 8):
            wide = lambda x: np.ascontiguousarray(np.repeat(x, k, axis=1))      # noqa: E731
            time, relvel = _meeting(a, b, wide(level), wide(lo), wide(hi), wide(delay))
            assert _same_bits(time[:7], wide(want)[:7]) and np.isnan(time[7]).all() and np.isnan(relvel[7]).all(), (k, time[:, 0])
            assert np.all(relvel[:2] == 0) and not np.isnan(relvel[:7]).any(), relvel[:, 0]      # the two touches; the constant gap
        print("hand-made cases: %s" % time[:, 0])
        return
    worst = {"residual, of (c)": 0.0, "relvel, of its scale": 0.0}
    for n, k in SHAPES:
        a, b, delays = gg._family(family, n)
        level, lo, hi, delay, reached = _queries(family, a, b, delays, k, 300 + k)
        want, _, (t_lo, t_hi) = mr.meeting_ld(a, b, level, lo, hi, delay)
        time, relvel = _meeting(a, b, level, lo, hi, delay)
        assert np.array_equal(np.isnan(want), ~reached), (family, n, k)
        assert np.array_equal(np.isnan(time), ~reached) and np.array_equal(np.isnan(relvel), ~reached), (family, n, k, "the NaN mask")
        T = mr.tmax(a, b, delay)
        assert np.all(((time >= t_lo - 4 * EPS * T) & (time <= t_hi + 4 * EPS * T))[reached]), (family, n, k, "the sub-piece")
        ratio, v_ld = _bound_c(a, b, level, delay, time, None)
        verr = np.where(reached, np.abs(relvel - v_ld), 0) / np.maximum(tr.scales(a)[1], tr.scales(b)[1])
        print("%s %d x %d: %.1f %% reached, residual %.3f of (c), relvel %.2e of its scale" % (family, n, k, 100 * reached.mean(), ratio.max(), verr.max()))
        worst["residual, of (c)"] = max(worst["residual, of (c)"], float(ratio.max()))
        worst["relvel, of its scale"] = max(worst["relvel, of its scale"], float(verr.max()))
    print("%s: %s" % (family, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["residual, of (c)"] <= 1.0 and worst["relvel, of its scale"] <= 2e-13


# ---------------------------------------------------------------- 2. the identities of the returned time
def test_returned_time_identities():
    """rp_trajectory_eval(A, t) - rp_trajectory_eval(B, t - delay) - level within (c), and d_relvel bit for bit the difference of the two
    evaluators' velocities there."""
    worst = 0.0
    for family in FAMILIES:
        for n, k in SHAPES[1:]:
            a, b, delays = gg._family(family, n)
            level, lo, hi, delay, reached = _queries(family, a, b, delays, k, 400 + k)
            time, relvel = _meeting(a, b, level, lo, hi, delay)
            at = np.where(reached, time, 0.0)
            ea, eb = tg._eval(a, at, want=(True, True, False)), tg._eval(b, at - np.where(reached, delay, 0.0), want=(True, True, False))
            assert np.array_equal(np.isnan(time), ~reached) and np.array_equal(_bits((ea[1] - eb[1])[reached]), _bits(relvel[reached])), (family, n, k)
            worst = max(worst, float(_bound_c(a, b, level, delay, time, (ea[0] - eb[0]) - level)[0].max()))
    print("the evaluators' gap at the returned time minus the level: %.3f of (c); relvel is their velocities' difference bit for bit" % worst)
    assert worst <= 1.0


# ---------------------------------------------------------------- 3. NULL arguments and the NaN rule
def test_null_arguments_and_the_nan_rule():
    a, b, delays = gg._family("random", 257)
    level, lo, hi, delay, reached = _queries("random", a, b, delays, 7, 1)
    clean = _meeting(a, b, level, lo, hi, delay)
    inf, zero = np.full(lo.shape, np.inf), np.zeros(lo.shape)
    for args, explicit in (((None, lo, hi, delay), (zero, lo, hi, delay)), ((level, None, hi, delay), (level, -inf, hi, delay)),
                           ((level, lo, None, delay), (level, lo, inf, delay)), ((level, lo, hi, None), (level, lo, hi, zero)),
                           ((None, None, None, None), (zero, -inf, inf, zero))):
        got, want = _meeting(a, b, *args, k=7), _meeting(a, b, *explicit)
        assert _both_same(got, want), [x is None for x in args]
        print("NULL %s: %d of %d queries have a meeting" % ([x is None for x in args], int((~np.isnan(got[0])).sum()), got[0].size))
    assert _same_bits(_meeting(a, b, level, lo, hi, delay, relvel=False)[0], clean[0])
    assert (~np.isnan(_meeting(a, b, None, None, None, None, k=7)[0])).mean() > 0.05      # the NULL cases are not all NaN
    # NULL end velocities are zeros
    za, zb = [x.copy() for x in a], [x.copy() for x in b]
    for s in (za, zb):
        s[3][:], s[4][:] = 0.0, 0.0
    lz = mr.levels(za, zb, lo, hi, delay, 3)[0]
    assert _both_same(_meeting(za, zb, lz, lo, hi, delay, zero_vel=True), _meeting(za, zb, lz, lo, hi, delay))
    # the NaN rule: a duration of 0, -1, inf, NaN in either spline poisons its problem and no other; a NaN window end, a NaN or infinite
    # delay, a NaN or infinite level its own query and no other
    a, b, level, lo, hi, delay = [x.copy() for x in a], [x.copy() for x in b], level.copy(), lo.copy(), hi.copy(), delay.copy()
    a[6][3], b[7][64], a[6][130], b[7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    delay[12, 1], delay[13, 2], delay[14, 3] = np.nan, np.inf, -np.inf
    level[15, 1], level[16, 2], level[17, 3] = np.nan, np.inf, -np.inf
    bad = np.zeros((257, 7), dtype=bool)
    bad[[3, 64, 130, 256]] = True
    for at in ((10, 0), (200, 4), (11, 3), (12, 1), (13, 2), (14, 3), (15, 1), (16, 2), (17, 3)):
        bad[at] = True
    got = _meeting(a, b, level, lo, hi, delay)
    for x, ref in zip(got, clean):
        assert np.array_equal(np.isnan(x), bad | np.isnan(ref))
        assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad]))
    print("NULL arguments are their values bit for bit; the NaN rule touches its own problem or query only")


# ---------------------------------------------------------------- 4. reproducibility
def test_bits_depend_on_the_problem_and_its_query_only():
    for family in FAMILIES:
        a, b, delays = gg._family(family)
        level, lo, hi, delay, _ = _queries(family, a, b, delays, 7, 507)
        first = _meeting(a, b, level, lo, hi, delay)
        assert _both_same(first, _meeting(a, b, level, lo, hi, delay)), "differs from run to run"
        order = np.random.default_rng(5).permutation(N)
        moved = _meeting([x[order] for x in a], [x[order] for x in b], level[order], lo[order], hi[order], delay[order])
        assert _both_same(moved, [x[order] for x in first]), family
        for rows in (slice(0, 1), slice(0, 129), slice(256, N)):
            own = _meeting([x[rows] for x in a], [x[rows] for x in b], level[rows], lo[rows], hi[rows], delay[rows])
            assert _both_same(own, [x[rows] for x in first]), (family, rows)
        for at in (0, 3, 7):
            wide = lambda x, fill: np.ascontiguousarray(np.insert(x, at, fill, axis=1))      # noqa: E731
            eight = _meeting(a, b, wide(level, 0.3), wide(lo, 0.1), wide(hi, 0.2), wide(delay, 0.05))
            assert _both_same([np.delete(x, at, axis=1) for x in eight], first), (family, at)
    print("the same bits in any order, in any batch and in any launch shape")


# ---------------------------------------------------------------- 5. autograd
def _leaves(a, b, *queries):
    ins_a = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, a)}
    ins_b = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, b)}
    return ins_a, ins_b, [_t(x).requires_grad_() for x in queries]


def _run(va, vb, level, lo, hi, delay):
    six = lambda v: [v[nm] for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1", "vel0", "vel2")]      # noqa: E731
    return rp.trajectory_meeting(six(va), six(vb), level, lo, hi, delay)


def test_autograd_reverse_forward_and_duality():
    k = 7
    for family in FAMILIES:
        a, b, delays = gg._family(family)
        lv_np, lo_np, hi_np, dl_np, reached = _queries(family, a, b, delays, k, 8)
        ins_a, ins_b, (level, lo, hi, delay) = _leaves(a, b, lv_np, lo_np, hi_np, dl_np)
        rng = np.random.default_rng(9)
        keep = reached & mr.difference_is_a_yardstick(a, b, lv_np, dl_np, mr.meeting_ld(a, b, lv_np, lo_np, hi_np, dl_np)[0])
        gn = rng.standard_normal((N, k))
        g = _t(gn)
        time = _run(ins_a, ins_b, level, lo, hi, delay)
        dev_t, dev_v = _meeting(a, b, lv_np, lo_np, hi_np, dl_np)
        assert time.requires_grad and _same_bits(time.detach().cpu().numpy(), dev_t) and np.array_equal(np.isnan(dev_t), ~reached), family
        leaves = [ins_a[nm] for nm in NAMES] + [ins_b[nm] for nm in NAMES] + [level, delay]
        grads = torch.autograd.grad(time, leaves + [lo, hi], grad_outputs=g, retain_graph=True, allow_unused=True)
        assert all(x is None or not x.any() for x in grads[18:]), "lo and hi only choose the branch"
        got = [x.cpu().numpy() for x in grads[:18]]
        assert all(np.isfinite(x).all() for x in got) and all(np.all(x[~reached] == 0) for x in got[16:]), family
        # the composition by hand through the evaluator's entries: the same bits
        missing = ~reached
        t_a, t_b = np.where(missing, 0.0, dev_t), np.where(missing, 0.0, dev_t - dl_np)
        w = torch.where(_t(missing).bool(), torch.zeros_like(g), g / _t(dev_v)).cpu().numpy()
        hand_a = tg._vjp(a, t_a, (-w, None, None), want_tau=False)[0]
        hand_b, tau_bar = tg._vjp(b, t_b, (w, None, None))
        assert all(_same_bits(x, y) for x, y in zip(got, hand_a + hand_b + [w, -tau_bar])), family
        # against the longdouble derivative at the device's own times; the yardstick is the same composition on the float64 restatements
        flat = lambda r: r[0] + r[1] + [r[2], r[3]]      # noqa: E731
        ref = flat(mr.derivative_ld(a, b, dl_np, dev_t, gn))
        r64 = flat(mr.derivative_ld(a, b, dl_np, dev_t, gn, vjp=tr.vjp_f64, forward=tr.forward_f64, T=np.float64))
        restated, device = float(np.max(tr.normwise(r64, ref))), float(np.max(tr.normwise(got, ref)))
        print("%s: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # reverse mode against central differences of the device op, on the queries where those are a yardstick
        gk = np.where(keep, gn, 0.0)
        got_k = [x.cpu().numpy() for x in torch.autograd.grad(time, leaves, grad_outputs=_t(gk), retain_graph=True)]
        steps_a, steps_b, level_step, delay_step = mr.difference_steps(a, b, lv_np, dl_np)

        def F(sa, sb, lv, dl):
            return np.where(keep, gk * _meeting(sa, sb, lv, lo_np, hi_np, dl, relvel=False)[0], 0.0)

        fd, stable = [], np.ones(N, dtype=bool)

        def difference(up, dn, h):
            nonlocal stable
            stable &= ~(np.isnan(up).any(axis=1) | np.isnan(dn).any(axis=1))      # a kept query lost its meeting under the step
            return (up - dn) / h

        for which, steps in enumerate((steps_a, steps_b)):
            for f in range(8):
                up, dn = [x.copy() for x in (a, b)[which]], [x.copy() for x in (a, b)[which]]
                up[f], dn[f] = up[f] + steps[f], dn[f] - steps[f]
                pair = (F(up, b, lv_np, dl_np), F(dn, b, lv_np, dl_np)) if which == 0 else (F(a, up, lv_np, dl_np), F(a, dn, lv_np, dl_np))
                fd.append(difference(*pair, (up[f] - dn[f])[:, None]).sum(axis=1))
        up, dn = lv_np + level_step, lv_np - level_step
        fd.append(difference(F(a, b, up, dl_np), F(a, b, dn, dl_np), up - dn))
        up, dn = dl_np + delay_step, dl_np - delay_step
        fd.append(difference(F(a, b, lv_np, up), F(a, b, lv_np, dn), up - dn))
        rows = keep.any(axis=1) & stable
        err = float(np.max(tr.normwise([x[rows] for x in got_k], [x[rows] for x in fd])))
        print("%s: reverse mode against central differences of the device op: %.2e normwise over %.0f %% of the reached queries, %.0f %% of the problems"
              % (family, err, 100 * keep.sum() / reached.sum(), 100 * rows.mean()))
        assert err <= 1e-6 and rows.mean() > 0.9 and keep.sum() >= 0.4 * reached.sum(), family
        # forward mode
        da, db = [_t(d) for d in tg._tangents(N, k, 10)[0]], [_t(d) for d in tg._tangents(N, k, 11)[0]]
        q_dot = [_t(rng.standard_normal((N, k))) for _ in range(4)]
        detached = [x.detach() for x in (level, lo, hi, delay)]
        with fwAD.dual_level():
            dual_a = {nm: fwAD.make_dual(ins_a[nm].detach(), d) for nm, d in zip(NAMES, da)}
            dual_b = {nm: fwAD.make_dual(ins_b[nm].detach(), d) for nm, d in zip(NAMES, db)}
            got_dot = fwAD.unpack_dual(_run(dual_a, dual_b, *[fwAD.make_dual(x, d) for x, d in zip(detached, q_dot)])).tangent.cpu().numpy()

        def f(*xs):
            return _run(dict(zip(NAMES, xs[:8])), dict(zip(NAMES, xs[8:16])), *xs[16:])
        primals = tuple(ins_a[nm].detach() for nm in NAMES) + tuple(ins_b[nm].detach() for nm in NAMES) + tuple(detached)
        _, func_dot = torch.func.jvp(f, primals, tuple(da) + tuple(db) + tuple(q_dot))
        assert _same_bits(func_dot.cpu().numpy(), got_dot) and np.array_equal(np.isnan(got_dot), missing), family
        dan, dbn, qn = [d.cpu().numpy() for d in da], [d.cpu().numpy() for d in db], [d.cpu().numpy() for d in q_dot]
        pa = tg._jvp(a, t_a, dan, None, want=(True, False, False))[0]
        pb = tg._jvp(b, t_b, dbn, -qn[3], want=(True, False, False))[0]
        hand = torch.where(_t(missing).bool(), torch.full_like(g, float("nan")), (q_dot[0] - _t(pa) + _t(pb)) / _t(dev_v)).cpu().numpy()
        assert _same_bits(hand, got_dot), family
        zap = lambda x: np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x)      # noqa: E731
        dot_ld = zap(mr.derivative_jvp_ld(a, b, dl_np, dev_t, dan, dbn, qn[0], qn[3]))
        dot64 = zap(mr.derivative_jvp_ld(a, b, dl_np, dev_t, dan, dbn, qn[0], qn[3], jvp=tr.jvp_f64, forward=tr.forward_f64, T=np.float64))
        restated, device = float(np.max(tr.normwise([dot64], [dot_ld]))), float(np.max(tr.normwise([zap(got_dot)], [dot_ld])))
        print("%s: forward mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # duality between the two modes: <g, J u> = <J^T g, u>
        left_terms = [np.where(missing, 0, gn.astype(LD) * zap(got_dot))]
        right_terms = [x.astype(LD) * d for x, d in zip(got, dan + dbn + [qn[0], qn[3]])]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        size = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, family
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(_run(ins_a, ins_b, level, lo, hi, delay)) ** 2).sum(), ins_a["pos1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        if family != "random":
            continue
        # a (k,) query is every problem's; all four None: k = 1, level 0 on the whole common domain; six tensors: vel0 / vel2 are zeros
        z = np.zeros(N)
        flat_a, flat_b = [a[0], a[1], a[2], z, z, a[5], a[6], a[7]], [b[0], b[1], b[2], z, z, b[5], b[6], b[7]]
        six_a = [ins_a[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        six_b = [ins_b[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        row_level, row_delay = np.array([0.5, -1.0, 0.0]), np.array([0.01, -0.02, 0.0])
        tl, td = _t(row_level).requires_grad_(), _t(row_delay).requires_grad_()
        o = rp.trajectory_meeting(six_a, six_b, tl, None, None, td)
        want = _meeting(flat_a, flat_b, np.repeat(row_level[None, :], N, axis=0), None, None, np.repeat(row_delay[None, :], N, axis=0))[0]
        assert _same_bits(o.detach().cpu().numpy(), want) and (~np.isnan(want)).mean() > 0.05
        g_level, g_delay = torch.autograd.grad(torch.nan_to_num(o).sum(), [tl, td])
        assert g_level.shape == (3,) and g_delay.shape == (3,) and bool(g_level.isfinite().all()) and bool(g_delay.isfinite().all())
        whole = rp.trajectory_meeting(six_a, six_b)
        assert whole.shape == (N, 1) and _same_bits(whole.cpu().numpy(), _meeting(flat_a, flat_b, None, None, None, None, k=1)[0])
    # a time that sits on the window's start because the gap is at the level there moves with the level by 1 / relvel, not with lo
    a, b, lv_np, lo_np, hi_np, dl_np, want = mr.hand_made()
    ins_a, ins_b, (level, lo, hi, delay) = _leaves(a, b, lv_np, lo_np, hi_np, dl_np)
    time = _run(ins_a, ins_b, level, lo, hi, delay)
    g_level, g_lo = torch.autograd.grad(time[3, 0], [level, lo], allow_unused=True)
    relvel = _meeting(a, b, lv_np, lo_np, hi_np, dl_np)[1][3, 0]
    assert time[3, 0].item() == lo_np[3, 0] and g_level[3, 0].item() == 1.0 / relvel and (g_lo is None or not g_lo.any()), (g_level[3, 0].item(), relvel)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. through the solves
def test_the_pipeline_against_central_differences():
    """min_time_meeting on the 300 golden problems against themselves 25 lower and later, against central differences of itself in pos1 of
    each vehicle, on converged finite queries where those are a yardstick: section 15's pipeline bound, median < 1e-5 and 95 % < 1e-3."""
    n, k = N, 8
    pos = gg._golden_positions(n)
    xa = [_t(pos[:, c]).requires_grad_() for c in range(3)]
    xb = [_t(pos[:, c] - 25.0).requires_grad_() for c in range(3)]

    def pipeline(pa, pb, *queries):
        return rp.min_time_meeting(pa, pb, *queries, gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(xa, xb)
    assert len(first) == 3 and first[0].shape == (n, 1) and len(first[1]) == 5 and len(first[2]) == 5
    sols = [[t.cpu().numpy() for t in s[:3]] for s in first[1:]]
    conv = np.ones(n, dtype=bool)
    for s, status in zip(sols, (first[1][4], first[2][4])):
        conv &= np.isfinite(np.stack(s, 1)).all(1) & (s[1] > 0) & (s[2] > 0) & ((status & capi.ST_CONVERGED) != 0).cpu().numpy()
    print("%d of %d pairs converged" % (int(conv.sum()), n))
    assert conv.mean() > 0.95
    z = np.zeros(n)
    a = [np.where(conv, x, 1.0) for x in (pos[:, 0], pos[:, 1], pos[:, 2], z, z) + tuple(sols[0])]
    b = [np.where(conv, x, 1.0) for x in (pos[:, 0] - 25, pos[:, 1] - 25, pos[:, 2] - 25, z, z) + tuple(sols[1])]
    dl_np = gr.delays(a, b, k, 23, follow=True)      # fixed queries: they do not move with the solutions
    lo_np, hi_np = gr.windows(a, b, dl_np, 24)
    lv_np, reached, _ = mr.levels(a, b, lo_np, hi_np, dl_np, 25)
    queries = [_t(x) for x in (lv_np, lo_np, hi_np, dl_np)]
    time = pipeline(xa, xb, *queries)[0]
    got = time.detach().cpu().numpy()
    finite = conv[:, None] & np.isfinite(got)
    keep_np = finite & reached & mr.difference_is_a_yardstick(a, b, lv_np, dl_np, np.where(finite, got, np.nan))
    print("%.0f %% of the queries are converged and finite (%.0f %% reached by the restatement); %.0f %% of those pass the mask"
          % (100 * finite.mean(), 100 * reached.mean(), 100 * keep_np.sum() / finite.sum()))
    assert np.array_equal(finite[conv], reached[conv]) and keep_np.sum() > 0.5 * finite.sum()
    wt = _t(np.random.default_rng(26).uniform(0.5, 1.5, (n, k)))
    keep = _t(keep_np).bool()
    rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
    grads = torch.autograd.grad(rows(time).sum(), [xa[1], xb[1]])
    some = _t(keep_np.any(axis=1)).bool()
    h = 1e-4
    for which, vehicle in enumerate("ab"):
        with torch.no_grad():
            up, dn = [list(xa), list(xb)], [list(xa), list(xb)]
            up[which][1], dn[which][1] = up[which][1] + h, dn[which][1] - h
            fd = (rows(pipeline(up[0], up[1], *queries)[0]) - rows(pipeline(dn[0], dn[1], *queries)[0])) / (2 * h)
        ok = some & torch.isfinite(fd) & torch.isfinite(grads[which])
        rel = ((grads[which] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]
        print("  d time / d pos1 of %s against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% of the problems)"
              % (vehicle, rel.median(), rel.quantile(0.95), 100 * float(ok.float().mean())))
        assert float(ok.float().mean()) > 0.5 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, vehicle
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
