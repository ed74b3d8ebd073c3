"""The cases of tests/test_gpu_crossing.py, each run in a fresh process (`python tests/crossing_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound is
what it is: DESIGN.md section 14."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import crossing_ref as cr  # noqa: E402
import end_velocity_ref as er  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV, BIG, NS = tg.DEV, tg.BIG, tg.NS
KS = (1, 2, 33, 64, 65, 200)
LD = np.longdouble
EPS = np.finfo(np.float64).eps
FAMILIES = ("solved", "random", "rest")
NAMES = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")
_t, _bits, _same_bits, _head, Out = tg._t, tg._bits, tg._same_bits, tg._head, tg.Out


def _family(name):
    """One spline of BIG problems: trajectory_gpu_cases' device-solved (kappa = 0.1) and random ones, and rest-to-rest random ones
    (vel0 = vel2 = 0 exactly: a velocity root on s = 0)."""
    if name == "solved":
        return tg._families()["solved"]
    return tr.random_states(BIG, 5) if name == "random" else cr.rest_to_rest(BIG, 6)


def _cross(sp, lv, want_vel=True, zero_vel=False):
    n, k = lv.shape
    ts, tl = [_t(a) for a in sp], _t(lv)
    time, vel = Out(n, k), Out(n, k) if want_vel else None
    addr = [t.data_ptr() for t in ts]
    if zero_vel:
        addr[3] = addr[4] = 0
    capi.trajectory_crossing(0, 0, n, k, addr, tl.data_ptr(), time.ptr, vel.ptr if vel else 0)
    torch.cuda.synchronize()
    return time.get(), vel.get() if vel else None


def _levels(sp, k, seed):
    """levels() with the exact columns: pos0 in column 0 (k == 1: in the even rows), pos1 in column 1 of the problems whose knot
    velocity is > 0.01 X / T.  Returns (levels, the mask of the exact entries)."""
    lv = cr.levels(sp, k, seed)
    exact = np.zeros(lv.shape, dtype=bool)
    exact[:, 0] = True if k > 1 else np.arange(len(lv)) % 2 == 0
    lv[:, 0] = np.where(exact[:, 0], sp[0], lv[:, 0])
    if k > 1:
        X, T = tr.scales(sp)[0][:, 0], sp[6] + sp[7]
        exact[:, 1] = sp[5] > 0.01 * X / T
        lv[:, 1] = np.where(exact[:, 1], sp[1], lv[:, 1])
    return lv, exact


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    sp_big = _family(family)
    X_big, V_big, T_big = tr.scales(sp_big)[0], tr.scales(sp_big)[1], (sp_big[6] + sp_big[7])[:, None]
    worst = {"residual of its bound": 0.0, "vel of its bound": 0.0, "time from the definition's, of T": 0.0}
    for k in KS:
        lv_big, exact_big = _levels(sp_big, k, 100 + k)
        want_big, _, (lo_big, hi_big) = cr.crossing_ld(sp_big, lv_big)
        for n in NS:
            sp, lv, want, X, V, T = _head(sp_big, n), lv_big[:n], want_big[:n], X_big[:n], V_big[:n], T_big[:n]
            time, vel = _cross(sp, lv)
            missing = np.isnan(time)
            assert np.array_equal(missing, np.isnan(want)), (family, n, k, "(a) the NaN mask")
            assert np.array_equal(np.isnan(vel), missing), (family, n, k, "(d) vel is NaN where the time is")
            inside = (time >= lo_big[:n] - 4 * EPS * T) & (time <= hi_big[:n] + 4 * EPS * T)
            assert inside[~missing & ~exact_big[:n]].all(), (family, n, k, "(b) the piece")
            zero = exact_big[:n, 0]
            assert np.all(_bits(time[zero, 0]) == 0), (family, n, k, "level == pos0 gives +0.0")
            pos, v_ld, _ = tr.forward_ld(sp, np.where(missing, 0.0, time))
            ratio = np.where(missing, 0, np.abs(pos - lv.astype(LD)) / (1e-13 * X + 4 * EPS * T * np.abs(v_ld)))
            worst["residual of its bound"] = max(worst["residual of its bound"], float(ratio.max()))
            worst["vel of its bound"] = max(worst["vel of its bound"], float(np.where(missing, 0, np.abs(vel - v_ld) / (1e-13 * V)).max()))
            worst["time from the definition's, of T"] = max(worst["time from the definition's, of T"],
                                                            float(np.where(missing, 0, np.abs(time - want) / T).max()))
            if n == 65 or (n, k) == (BIG, 200):      # (e) a NULL d_vel: the same time bits
                only, none = _cross(sp, lv, want_vel=False)
                assert none is None and _same_bits(only, time), (family, n, k)
    print("%s over %s x %s: %s" % (family, NS, KS, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst["residual of its bound"] <= 1.0, "(c)"
    assert worst["vel of its bound"] <= 1.0, "(d)"
    # (e) the NaN rule: a duration of 0, -1, inf, NaN poisons its problem and no other; a NaN level its own query and no other
    n, k = 257, 33
    sp = [a.copy() for a in _head(sp_big, n)]
    lv = cr.levels(sp, k, 1)
    clean = _cross(sp, lv)
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    hit = [(row, int(np.argmax(~np.isnan(clean[0][row])))) for row in (10, 200)]      # a reached query of each of two rows
    assert all(not np.isnan(clean[0][h]) for h in hit)
    lv[hit[0]] = lv[hit[1]] = np.nan
    bad_rows = np.zeros(n, dtype=bool)
    bad_rows[[3, 64, 130, 256]] = True
    bad = np.repeat(bad_rows[:, None], k, axis=1)
    bad[hit[0]] = bad[hit[1]] = True
    for got, ref in zip(_cross(sp, lv), clean):
        assert np.array_equal(np.isnan(got), bad | np.isnan(ref)), family
        assert np.array_equal(_bits(got[~bad]), _bits(ref[~bad])), family
    # NULL end velocities are zeros
    if family == "rest":
        a, b = _cross(_head(sp_big, 65), lv_big[:65], zero_vel=True), _cross(_head(sp_big, 65), lv_big[:65])
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


# ---------------------------------------------------------------- 2. the batch entry
def test_batch_entry_equals_the_stateless_one():
    orc = Oracle()
    n = 4097
    rng = np.random.default_rng(12)
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
                low, high = np.minimum(sp[0], sp[2])[:, None], np.maximum(sp[0], sp[2])[:, None]
                for k in (1, 33, 64, 200):
                    lv = low - 0.1 * (high - low) + rng.uniform(size=(n, k)) * 1.2 * (high - low)      # a tenth of them beyond each end
                    tl = _t(lv)
                    time, velo = Out(n, k), Out(n, k)
                    b.crossing_device(tl.data_ptr(), k, time.ptr, velo.ptr)
                    b.sync()
                    got = (time.get(), velo.get())
                    want = _cross(sp, lv)
                    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), (variant, dtype, vel, k)
                    only = Out(n, k)
                    b.crossing_device(tl.data_ptr(), k, only.ptr)
                    b.sync()
                    assert _same_bits(only.get(), got[0])
                reached = float((~np.isnan(got[0])).mean())
                print("variant %d dtype %d vel %s: the batch entry's bits are the stateless entry's; %.0f %% of the levels reached" % (variant, dtype, vel, 100 * reached))
                assert reached > 0.5


# ---------------------------------------------------------------- 3. reproducibility
def test_bits_depend_on_the_problem_and_the_level_only():
    for family in FAMILIES:
        sp_big = _family(family)
        for k in KS:
            lv_big, _ = _levels(sp_big, k, 500 + k)
            first = _cross(sp_big, lv_big)
            again = _cross(sp_big, lv_big)
            assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1]), "differs from run to run"
            for n in NS[:-1]:
                small = _cross(_head(sp_big, n), lv_big[:n])
                assert _same_bits(small[0], first[0][:n]) and _same_bits(small[1], first[1][:n]), (family, n, k)
            roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
            moved = _cross([roll(a) for a in sp_big], roll(lv_big))
            for a, b in zip(moved, first):
                assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (family, k)
    # ... nor on which of a block's trips the problem is in: more trips than the grid's cap
    sp = tr.random_states(tg.GRID_N, 77)
    for k in tg.GRID_KS:
        tg.rows_equal_their_own_batch(("crossing", k), lambda s, lv: list(_cross(s, lv)), sp, _levels(sp, k, 800 + k)[0])


# ---------------------------------------------------------------- 4. autograd
def _stable_pieces(sp, lv, piece):
    """Whether the definition (longdouble) keeps each query's piece under every one of the eighteen steps of the central differences."""
    steps, level_step = cr.difference_steps(sp, lv)
    same = np.ones(lv.shape, dtype=bool)
    for sign in (1.0, -1.0):
        for f in range(8):
            moved = [np.asarray(a, dtype=LD) for a in sp]
            moved[f] = moved[f] + sign * steps[f]
            same &= cr.crossing_ld(moved, lv)[1] == piece
        same &= cr.crossing_ld(sp, lv.astype(LD) + sign * level_step)[1] == piece
    return same


def test_autograd_reverse_forward_and_duality():
    """Reverse and forward mode are the documented compositions bit for bit; both hold against the longdouble implicit derivative at the
    device's own times to ten times what the float64 restatement of the evaluator's derivative kernels holds on the same inputs
    (section 13 case 3's rule); reverse mode against central differences of the device op (step 1e-6 max(|x|, 1), 1e-6 normwise) on the
    queries with |vel| >= 0.01 X / T (their levels are at least 1 % of their piece's range from its ends by construction) at which the
    difference quotient is a yardstick -- crossing_ref.difference_is_a_yardstick, and the definition keeps the query's piece under every
    step: without those two the LONGDOUBLE quotient of the LONGDOUBLE crossing misses 1e-6 by itself (tests/test_crossing_cpu.py)."""
    n, k = 257, 33
    for family in FAMILIES:
        sp = _head(_family(family), n)
        lv, reached, _ = cr.levels(sp, k, 8, with_reached=True)
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
        L = _t(lv).requires_grad_()
        g = _t(np.random.default_rng(9).standard_normal((n, k)))

        def run(v, level):
            return rp.trajectory_crossing(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], level, vel0=v["vel0"], vel2=v["vel2"])

        time = run(ins, L)
        grads = torch.autograd.grad(time, [ins[nm] for nm in NAMES] + [L], grad_outputs=g, retain_graph=True)
        t_dev, v_dev = _cross(sp, lv)
        assert _same_bits(time.detach().cpu().numpy(), t_dev)
        missing = np.isnan(t_dev)
        assert np.array_equal(missing, ~reached)
        # the composition by hand: w = g / vel (0 where no crossing), level_bar = w, the evaluator's VJP at the times (0 there) for g_pos = -w
        tm, tv, miss = _t(np.where(missing, 0.0, t_dev)), _t(v_dev), _t(missing).bool()
        w = torch.where(miss, torch.zeros_like(g), g / tv)
        neg = (-w).contiguous()
        bars = [Out(n) for _ in range(8)]
        capi.trajectory_eval_vjp(0, 0, n, k, [ins[nm].data_ptr() for nm in NAMES], tm.data_ptr(), neg.data_ptr(), 0, 0, [o.ptr for o in bars], 0)
        torch.cuda.synchronize()
        hand = [o.get() for o in bars] + [w.cpu().numpy()]
        got = [x.cpu().numpy() for x in grads]
        assert all(_same_bits(a, b) for a, b in zip(got, hand)), family
        # an unreached level contributes exactly 0 whatever its upstream gradient, and the gradients are finite
        assert np.all(got[8][missing] == 0) and all(np.isfinite(x).all() for x in got), family
        masked = torch.autograd.grad(time, [ins[nm] for nm in NAMES] + [L], grad_outputs=torch.where(miss, torch.zeros_like(g), g), retain_graph=True)
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(masked, got)), family
        # forward mode by hand: the evaluator's JVP with no tangent on the time, pos_dot only; (level_dot - pos_dot) / vel, NaN where no crossing
        dots, ldot = tg._tangents(n, k, 10)
        dts, tl = [_t(d) for d in dots], _t(ldot)
        pd = Out(n, k)
        capi.trajectory_eval_jvp(0, 0, n, k, [ins[nm].data_ptr() for nm in NAMES], tm.data_ptr(), [d.data_ptr() for d in dts], 0, pd.ptr, 0, 0)
        torch.cuda.synchronize()
        want_dot = torch.where(miss, torch.full_like(g, float("nan")), (tl - _t(pd.get())) / tv).cpu().numpy()
        with fwAD.dual_level():
            dual = {nm: fwAD.make_dual(ins[nm].detach(), d) for nm, d in zip(NAMES, dts)}
            got_dot = fwAD.unpack_dual(run(dual, fwAD.make_dual(L.detach(), tl))).tangent.cpu().numpy()
        assert _same_bits(got_dot, want_dot), family

        def f(*xs):
            return run(dict(zip(NAMES, xs[:8])), xs[8])
        _, func_dot = torch.func.jvp(f, tuple(ins[nm].detach() for nm in NAMES) + (L.detach(),), tuple(dts) + (tl,))
        assert _same_bits(func_dot.cpu().numpy(), want_dot), family
        # against the longdouble implicit derivative at the device's own times; the yardstick is the evaluator's float64 restatement
        rows = reached.any(axis=1)
        gn = g.cpu().numpy()
        bars_ld, w_ld = cr.derivative_ld(sp, t_dev, gn)
        tau0 = np.where(missing, 0.0, t_dev)
        with np.errstate(all="ignore"):
            w64 = np.where(missing, 0.0, gn / tr.forward_f64(sp, tau0)[1])
        zero = np.zeros((n, k))
        bars64, _ = tr.vjp_f64(sp, tau0, -w64, zero, zero)
        pick = lambda xs: [np.asarray(x)[rows] for x in xs]      # noqa: E731
        restated = float(np.max(tr.normwise(pick(bars64 + [w64]), pick(bars_ld + [w_ld]))))
        device = float(np.max(tr.normwise(pick(got), pick(bars_ld + [w_ld]))))
        print("%s: reverse mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        dot_ld = np.where(missing, LD(0), cr.derivative_jvp_ld(sp, t_dev, dots, ldot))
        with np.errstate(all="ignore"):
            dot64 = np.where(missing, 0.0, (ldot - tr.jvp_f64(sp, tau0, dots, zero)[0]) / tr.forward_f64(sp, tau0)[1])
        restated = float(np.max(tr.normwise(pick([dot64]), pick([dot_ld]))))
        device = float(np.max(tr.normwise(pick([np.where(missing, 0.0, got_dot)]), pick([dot_ld]))))
        print("%s: forward mode against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, restated, device, 10 * restated))
        assert device <= 10 * restated, family
        # reverse mode against central differences of the device op
        want_t, piece, _ = cr.crossing_ld(sp, lv)
        X, T = tr.scales(sp)[0], (sp[6] + sp[7])[:, None]
        v_ld = tr.forward_ld(sp, tau0)[1]
        slow = reached & (np.abs(v_ld) >= 0.01 * X / T)
        keep = slow & cr.difference_is_a_yardstick(sp, t_dev, lv) & _stable_pieces(sp, lv, piece)
        kept = _t(keep).bool()

        def loss_rows(v, level):
            return torch.where(kept, g * run(v, level), torch.zeros_like(g))

        mine = torch.autograd.grad(loss_rows(ins, L).sum(), [ins[nm] for nm in NAMES] + [L])
        steps, level_step = cr.difference_steps(sp, lv)
        fd = []
        with torch.no_grad():
            for nm, h in zip(NAMES, steps):
                h = _t(h)
                up, dn = dict(ins), dict(ins)
                up[nm], dn[nm] = ins[nm] + h, ins[nm] - h
                fd.append(((loss_rows(up, L) - loss_rows(dn, L)).sum(1) / (2 * h)).cpu().numpy())
            h = _t(level_step)
            fd_level = ((loss_rows(ins, L + h) - loss_rows(ins, L - h)) / (2 * h)).cpu().numpy()
        assert all(np.isfinite(x).all() for x in fd + [fd_level]), family
        some = keep.any(axis=1)
        e_par = float(np.max(tr.normwise([x.cpu().numpy()[some] for x in mine[:8]], [x[some] for x in fd])))
        e_lev = float(np.max(tr.normwise([mine[8].cpu().numpy()[some]], [fd_level[some]])))
        print("%s: reverse mode against central differences of the device op on %.0f %% of the queries (%.0f %% have |vel| >= 0.01 X / T), normwise: "
              "spline inputs %.2e, level %.2e" % (family, 100 * keep.mean(), 100 * slow.mean(), e_par, e_lev))
        assert keep.mean() > 0.5 and e_par < 1e-6 and e_lev < 1e-6, family
        # duality between the two modes: <g, J u> = <J^T g, u>
        gl = np.where(missing, 0.0, gn).astype(LD)
        left = float((gl * np.where(missing, 0.0, got_dot)).sum())
        terms = [x.astype(LD) * d for x, d in zip(got[:8], dots)] + [got[8].astype(LD) * ldot]
        right = sum(float(x.sum()) for x in terms)
        size = sum(float(np.abs(x).sum()) for x in terms) + float(np.abs(gl * np.where(missing, 0.0, got_dot)).sum())
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, family
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(run(ins, L)) ** 2).sum(), ins["vel1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        # a (k,) level is every problem's; vel0 / vel2 of None are zeros
        row = _t(lv[0]).requires_grad_()
        o = rp.trajectory_crossing(*[ins[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")], row)
        z = np.zeros(n)
        assert _same_bits(o.detach().cpu().numpy(), _cross([sp[0], sp[1], sp[2], z, z, sp[5], sp[6], sp[7]], np.repeat(lv[:1], n, axis=0))[0])
        (g_row,) = torch.autograd.grad(torch.nan_to_num(o).sum(), row)
        assert g_row.shape == (k,)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the identity through the solve
def test_the_knot_crossing_moves_as_duration0():
    """level = pos1: the crossing is the knot, time = duration0, and d time = d duration0 in every input -- at tau = duration0,
    d pos / d pos1 = 1 and d pos / d duration0 = -vel.  4,096 monotone problems, kappa = 0.1, gap 1e-13."""
    orc = Oracle()
    n = 4096
    args = er.velocities(orc, 0, 0.1, n, 51)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}
    time, vel1, d0, d1, _, status = rp.min_time_crossing(x["pos0"], x["pos1"], x["pos2"], x["pos1"][:, None], vel0=x["vel0"], vel2=x["vel2"], gap_tol=1e-13)
    sol = [t.detach().cpu().numpy() for t in (vel1, d0, d1)]
    live = np.isfinite(np.stack(sol, 1)).all(1) & (sol[1] > 0) & (sol[2] > 0)
    sp = [np.where(live, a, 1.0) for a in (args[0], args[1], args[2], args[3], args[4]) + tuple(sol)]
    X, T = tr.scales(sp)[0][:, 0], sp[6] + sp[7]
    fine = live & ((status.cpu().numpy() & capi.ST_CONVERGED) != 0) & (sp[5] > 0.01 * X / T)
    print("%d of %d problems converged with a knot velocity above 0.01 X / T" % (int(fine.sum()), n))
    assert fine.mean() > 0.95
    t_dev = time.detach().cpu().numpy()[:, 0]
    assert not np.isnan(t_dev[fine]).any()
    tau = np.where(fine, t_dev, 0.5)[:, None]
    pos, v_ld, _ = tr.forward_ld(sp, tau)
    bound = (1e-13 * X + 4 * EPS * T * np.abs(v_ld[:, 0])).astype(np.float64)
    residual = np.abs(pos[:, 0] - sp[1].astype(LD)).astype(np.float64)
    away = np.abs(t_dev - sp[6]) * np.abs(sp[5])
    print("the knot crossing: residual %.3g of bound (c), |time - duration0| |vel1| %.3g of it" % (float((residual / bound)[fine].max()), float((away / bound)[fine].max())))
    assert np.all(residual[fine] <= bound[fine]) and np.all(away[fine] <= bound[fine])
    # the total derivatives
    total = torch.autograd.grad(time.sum(), [x[nm] for nm in names], retain_graph=True)
    expected = torch.autograd.grad(d0.sum(), [x[nm] for nm in names])
    total, expected = np.stack([t.cpu().numpy() for t in total], 1), np.stack([t.cpu().numpy() for t in expected], 1)
    # the terms of the chain rule: the crossing's own gradients, and those in (vel1, duration0, duration1) times the solve's Jacobian
    leaf = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
    level = _t(sp[1][:, None]).requires_grad_()
    own = rp.trajectory_crossing(leaf["pos0"], leaf["pos1"], leaf["pos2"], leaf["vel1"], leaf["duration0"], leaf["duration1"], level, vel0=leaf["vel0"], vel2=leaf["vel2"])
    bars = [t.cpu().numpy() for t in torch.autograd.grad(torch.nan_to_num(own).sum(), [leaf[nm] for nm in NAMES] + [level])]
    jac = rp.min_time_jacobian(*[x[nm].detach() for nm in names[:3]], vel0=x["vel0"].detach(), vel2=x["vel2"].detach(), gap_tol=1e-13)[5].cpu().numpy()
    fine &= np.isfinite(jac.reshape(n, -1)).all(1)
    assert fine.mean() > 0.95
    worst = 0.0
    for b in range(5):
        terms = np.stack([bars[b], bars[5] * jac[:, 0, b], bars[6] * jac[:, 1, b], bars[7] * jac[:, 2, b],
                          bars[8][:, 0] if b == 1 else np.zeros(n), expected[:, b]], 1)
        miss = np.abs(total[:, b] - expected[:, b]) / np.maximum(np.abs(terms).max(1), 1e-300)
        worst = max(worst, float(miss[fine].max()))
    print("d time / d (pos0, pos1, pos2, vel0, vel2) against d duration0: off by %.2e of the largest chain-rule term" % worst)
    assert worst < 1e-10
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. round trip on the device
def test_round_trip_and_the_pipeline_against_differences():
    orc = Oracle()
    n, k = 4096, 8
    args = tg._inputs(orc, 0.1, n)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}
    rng = np.random.default_rng(23)
    lv = args[0][:, None] + rng.uniform(0.05, 0.95, (n, k)) * (args[2] - args[0])[:, None]      # fixed levels between pos0 and pos2
    L = _t(lv).requires_grad_()
    wt = _t(rng.uniform(0.5, 1.5, (n, k)))

    def rows(v, level):
        out = rp.min_time_crossing(v["pos0"], v["pos1"], v["pos2"], level, vel0=v["vel0"], vel2=v["vel2"], gap_tol=1e-13)
        return wt * out[0], out

    loss, out = rows(x, L)
    time, vel1, d0, d1, _, status = out
    # trajectory_eval at the returned times gives the level back
    reached = ~torch.isnan(time.detach())
    with torch.no_grad():
        pos, vel, _ = rp.trajectory_eval(x["pos0"], x["pos1"], x["pos2"], vel1, d0, d1, torch.where(reached, time, torch.zeros_like(time)), vel0=x["vel0"], vel2=x["vel2"])
    sol = [t.detach().cpu().numpy() for t in (vel1, d0, d1)]
    live = np.isfinite(np.stack(sol, 1)).all(1) & (sol[1] > 0) & (sol[2] > 0)
    sp = [np.where(live, a, 1.0) for a in tuple(args) + tuple(sol)]
    X, T = tr.scales(sp)[0], (sp[6] + sp[7])[:, None]
    ok_q = reached.cpu().numpy() & live[:, None]
    ratio = np.abs(pos.cpu().numpy() - lv) / (1e-13 * X + 4 * EPS * T * np.abs(vel.cpu().numpy()))
    print("trajectory_eval(trajectory_crossing(level)) - level: %.3g of bound (c), on %.0f %% of the queries" % (float(ratio[ok_q].max()), 100 * ok_q.mean()))
    assert ok_q.mean() > 0.9 and float(ratio[ok_q].max()) <= 1.0
    # the whole pipeline against central differences of itself
    grads = torch.autograd.grad(torch.where(reached, loss, torch.zeros_like(loss)).sum(), [x[nm] for nm in names] + [L])
    conv = ((status & capi.ST_CONVERGED) != 0) & _t(live).bool()
    ok = conv & torch.isfinite(torch.stack(grads[:5], 1)).all(1) & torch.isfinite(grads[5]).all(1)
    h = 1e-4
    stats = []
    with torch.no_grad():
        for i, nm in enumerate(names):
            up, dn = dict(x), dict(x)
            up[nm], dn[nm] = x[nm] + h, x[nm] - h
            diff = torch.where(reached, rows(up, L)[0] - rows(dn, L)[0], torch.zeros_like(loss))
            fd = diff.sum(1) / (2 * h)
            keep = ok & torch.isfinite(fd)
            stats.append((nm, ((grads[i] - fd).abs() / fd.abs().clamp(min=1e-3))[keep], float(keep.float().mean())))
        fd = (rows(x, L + h)[0] - rows(x, L - h)[0]) / (2 * h)
        keep = ok[:, None] & reached & torch.isfinite(fd)
        stats.append(("level", ((grads[5] - fd).abs() / fd.abs().clamp(min=1e-3))[keep], float(keep.float().mean())))
    print("%d of %d problems converged and finite" % (int(ok.sum()), n))
    for nm, rel, share in stats:
        print("  d / d %-5s against central differences of the pipeline: median %.2e, 95 %% %.2e (%.0f %% kept)" % (nm, rel.median(), rel.quantile(0.95), 100 * share))
    assert ok.float().mean() > 0.95
    for nm, rel, share in stats:
        assert share > 0.75 and rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, nm
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
