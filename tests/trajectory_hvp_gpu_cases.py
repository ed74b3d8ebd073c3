"""The cases of tests/test_gpu_trajectory_hvp.py, each run in a fresh process (`python tests/trajectory_hvp_gpu_cases.py <case>`): torch must
initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py).  Not collected by pytest (no test_ prefix on
the file).  What is checked, and why each bound is what it is: DESIGN.md section 17."""
import itertools
import os
import sys

import trajectory_gpu_cases as tc      # first: it initialises torch's HIP runtime on import, and puts the repository on sys.path

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import rocket_path_amd as rp  # noqa: E402
import trajectory_hvp_ref as hr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV, NS, KS, BIG = tc.DEV, tc.NS, tc.KS, tc.BIG
_t, _same_bits, _bits, _head, Out = tc._t, tc._same_bits, tc._bits, tc._head, tc.Out
NAMES = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")
LD = np.longdouble


def _hvp(sp, tau, g, dots, tdot, want_bars=(True,) * 8, want_tau=True, zero_vel=False):
    """g: three (n, k) arrays or None each (NULL pointers); dots: eight arrays of n or None each, or None (a NULL table); tdot (n, k) or
    None.  Returns (eight bar_dots or None each, tau_bar_dot or None)."""
    n, k = tau.shape
    ts, tt = [_t(a) for a in sp], _t(tau)
    gs = [_t(x) if x is not None else None for x in g]
    ds = [_t(x) if x is not None else None for x in dots] if dots is not None else None
    td = _t(tdot) if tdot is not None else None
    bars = [Out(n) if w else None for w in want_bars]
    tb = Out(n, k) if want_tau else None
    addr = [t.data_ptr() for t in ts]
    if zero_vel:
        addr[3] = addr[4] = 0
    capi.trajectory_eval_hvp(0, 0, n, k, addr, tt.data_ptr(), *[x.data_ptr() if x is not None else 0 for x in gs],
                             [x.data_ptr() if x is not None else 0 for x in ds] if ds is not None else None,
                             td.data_ptr() if td is not None else 0, [o.ptr if o else 0 for o in bars], tb.ptr if tb else 0)
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars], tb.get() if tb else None


def _all(result):
    return result[0] + [result[1]]


def _finite_max(x):
    worst = float(np.max(x))
    assert np.isfinite(worst), "a NaN or infinite result"      # a max would drop it
    return worst


def _normwise(a, b):
    """The worst of trajectory_ref.normwise over the problems -- where a problem's reference is exactly 0 (no query in a segment), the
    norm of the difference itself -- and never a NaN."""
    a = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in a], axis=1)
    b = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in b], axis=1)
    miss, size = np.linalg.norm((a - b).astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    return _finite_max(miss / np.where(size > 0, size, 1.0))


# ---------------------------------------------------------------- 1. the entry against longdouble
def test_entry_against_longdouble_nulls_and_nan_rule():
    """Normwise per problem against the longdouble definition: the float64 restatement of the kernel's arithmetic and order first, on the
    same inputs on the CPU; the device is held to 10 x the restatement's worst (DESIGN.md section 12's margin).  Every NULL input equals
    explicit zeros bit for bit; an output not asked for is not written (sentinels behind every buffer); the NaN rule."""
    fam = tc._families()
    worst = [0.0, 0.0]      # [restatement, device]
    for name, sp_big in fam.items():
        for k in KS:
            tau_big = tr.query_times(sp_big, k, 200 + k)
            g_big = hr.gradients(BIG, k, 300 + k)
            dots_big, tdot_big = hr.directions(BIG, k, 400 + k)
            ld = _all(hr.hvp_ld(sp_big, tau_big, *g_big, dots_big, tdot_big))      # a problem's result is its own: the heads are rows of these
            f64 = _all(hr.hvp_f64(sp_big, tau_big, *g_big, dots_big, tdot_big))
            worst[0] = max(worst[0], _normwise(f64, ld))
            for n in NS:
                sp, tau = _head(sp_big, n), tau_big[:n]
                g, dots, tdot = [x[:n] for x in g_big], [x[:n] for x in dots_big], tdot_big[:n]
                full = _hvp(sp, tau, g, dots, tdot)
                worst[1] = max(worst[1], _normwise(_all(full), [x[:n] for x in ld]))
                if n != 65:
                    continue
                zero, zn = np.zeros((n, k)), np.zeros(n)
                for null in itertools.product((False, True), repeat=3):
                    if any(null):
                        a = _hvp(sp, tau, [None if z else x for x, z in zip(g, null)], dots, tdot)
                        e = _hvp(sp, tau, [zero if z else x for x, z in zip(g, null)], dots, tdot)
                        assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(e))), (k, null)
                for null in ((True,) * 8 + (False,), (False,) * 8 + (True,), (True, False) * 4 + (True,), (False, True) * 4 + (False,)):
                    a = _hvp(sp, tau, g, [None if z else x for x, z in zip(dots, null)], None if null[8] else tdot)
                    e = _hvp(sp, tau, g, [zn if z else x for x, z in zip(dots, null)], zero if null[8] else tdot)
                    assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(e))), (k, null)
                a, e = _hvp(sp, tau, g, None, tdot), _hvp(sp, tau, g, [zn] * 8, tdot)      # no table at all
                assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(e))), k
                # outputs not asked for change nothing in the others; NULL end velocities are zeros
                for bars_wanted, tau_wanted in (((True, False) * 4, False), ((False, True) * 4, True), ((False,) * 8, True)):
                    part = _hvp(sp, tau, g, dots, tdot, want_bars=bars_wanted, want_tau=tau_wanted)
                    assert (part[1] is None) == (not tau_wanted) and (part[1] is None or _same_bits(part[1], full[1]))
                    assert all((p is None) == (not w) and (p is None or _same_bits(p, f)) for p, f, w in zip(part[0], full[0], bars_wanted))
                sp0 = [a.copy() for a in sp]
                sp0[3][:] = 0.0
                sp0[4][:] = 0.0
                a, e = _hvp(sp0, tau, g, dots, tdot, zero_vel=True), _hvp(sp0, tau, g, dots, tdot)
                assert all(_same_bits(x, y) for x, y in zip(_all(a), _all(e)))
    print("hvp against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (worst[0], worst[1], 10 * worst[0]))
    assert worst[1] <= 10 * worst[0]
    # the NaN rule: a duration <= 0, inf or NaN poisons its problem and no other; a NaN tau or tau_dot its own tau_bar_dot, and the sums of
    # its problem over its segment
    n, k = 257, 33
    sp = [a.copy() for a in _head(fam["solved"], n)]
    tau = tr.query_times(sp, k, 1)
    g = hr.gradients(n, k, 2)
    dots, tdot = hr.directions(n, k, 3)
    clean = _hvp(sp, tau, g, dots, tdot)
    assert all(np.isfinite(x).all() for x in _all(clean))
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    tau[10, 5] = tau[200, 32] = np.nan      # a NaN tau is a query of segment 1
    tdot[50, 7] = tdot[90, 0] = np.nan      # (90, 0): tau = 0, segment 0
    bad_rows = np.zeros(n, dtype=bool)
    bad_rows[[3, 64, 130, 256]] = True
    bad = np.repeat(bad_rows[:, None], k, axis=1)
    bad[10, 5] = bad[200, 32] = bad[50, 7] = bad[90, 0] = True
    bars, tau_bar = _hvp(sp, tau, g, dots, tdot)
    assert np.array_equal(np.isnan(tau_bar), bad)
    assert np.array_equal(_bits(tau_bar[~bad]), _bits(clean[1][~bad]))
    seg1 = {i: bool(tau[i, j] >= sp[6][i]) for i, j in ((50, 7), (90, 0))}
    assert not seg1[90]
    touched = [3, 64, 130, 256, 10, 200, 50, 90]
    for f, b in enumerate(bars):
        assert np.isnan(b[bad_rows]).all(), f
        rest = np.delete(np.arange(n), touched)
        assert np.array_equal(_bits(b[rest]), _bits(clean[0][f][rest])), f
        assert np.isnan(b[[10, 200]]).all() == (f not in (0, 3)), f      # segment 1's sums reach everything but pos0 and vel0
        for i in (50, 90):      # segment 0's reach everything but pos2, vel2 and duration1
            assert np.isnan(b[i]) == (f not in ((0, 3) if seg1[i] else (2, 4, 7))), (f, i)


# ---------------------------------------------------------------- 2. reproducibility
def test_bits_do_not_depend_on_the_batch_or_the_run():
    fam = tc._families()
    for name, sp_big in fam.items():
        for k in KS:
            tau_big = tr.query_times(sp_big, k, 500 + k)
            g_big = hr.gradients(BIG, k, 600 + k)
            dots_big, tdot_big = hr.directions(BIG, k, 700 + k)
            big = _all(_hvp(sp_big, tau_big, g_big, dots_big, tdot_big))
            again = _all(_hvp(sp_big, tau_big, g_big, dots_big, tdot_big))
            assert all(_same_bits(x, y) for x, y in zip(big, again)), "the HVP differs from run to run"
            for n in NS[:-1]:
                small = _hvp(_head(sp_big, n), tau_big[:n], [x[:n] for x in g_big], [x[:n] for x in dots_big], tdot_big[:n])
                for a, b in zip(_all(small), big):
                    assert _same_bits(a, b[:n]), (name, n, k)
            # ... nor on where in a batch the problem sits: problem 0 again as the last of 4097
            roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
            m = _hvp([roll(a) for a in sp_big], roll(tau_big), [roll(x) for x in g_big], [roll(x) for x in dots_big], roll(tdot_big))
            for a, b in zip(_all(m), big):
                assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (name, k)
    # ... nor on which of a block's trips the problem is in: more trips than the grid's cap
    sp = tr.random_states(tc.GRID_N, 77)
    for k in tc.GRID_KS:
        dots, tdot = hr.directions(tc.GRID_N, k, 820 + k)
        tc.rows_equal_their_own_batch(("hvp", k), lambda s, t, g, d, td: _all(_hvp(s, t, g, d, td)), sp, tr.query_times(sp, k, 800 + k),
                                      hr.gradients(tc.GRID_N, k, 810 + k), dots, tdot)


# ---------------------------------------------------------------- 3. identities on the device
def test_translation_symmetry_and_linearity_on_the_device():
    fam = tc._families()
    worst_sym = worst_lin = 0.0
    for name, sp_big in fam.items():
        for k in KS:
            for n in (65, BIG) if k in (33, 64) else (257,):
                sp = _head(sp_big, n)
                tau = tr.query_times(sp, k, 800 + k)
                g = hr.gradients(n, k, 900 + k)
                u, v = hr.directions(n, k, 1000 + k), hr.directions(n, k, 1100 + k)
                # the spline moved as a whole: +-0 in every output, given as ones, and with the zeros given as NULL
                zero = np.zeros((n, k))
                for dots, tdot in ((hr.translation(n), zero), ([x if f < 3 else None for f, x in enumerate(hr.translation(n))], None)):
                    for out in _all(_hvp(sp, tau, g, dots, tdot)):
                        assert np.all(out == 0.0), (name, n, k)
                # u^T H[g] v = v^T H[g] u: both sides hold to the ~1e-14 normwise of the check against longdouble, so by Cauchy-Schwarz their
                # difference to a few times that of the sum of |terms| for these random directions: 1e-12, the bound of section 13's duality
                left, size_l = hr.bilinear(*_hvp(sp, tau, g, *v), *u)
                right, size_r = hr.bilinear(*_hvp(sp, tau, g, *u), *v)
                worst_sym = max(worst_sym, _finite_max(np.abs(left - right) / (size_l + size_r)))
                # linear in g: g_pos alone plus g_vel alone is both, to 1e-12 of the sum of |terms| (the three results, element by element)
                both = _all(_hvp(sp, tau, [g[0], g[1], None], *v))
                only_p = _all(_hvp(sp, tau, [g[0], None, None], *v))
                only_v = _all(_hvp(sp, tau, [None, g[1], None], *v))
                for a, b, c in zip(only_p, only_v, both):
                    size = (np.abs(a) + np.abs(b) + np.abs(c)).astype(LD).reshape(n, -1).sum(axis=1)
                    miss = np.abs(a.astype(LD) + b.astype(LD) - c.astype(LD)).reshape(n, -1).sum(axis=1)
                    worst_lin = max(worst_lin, _finite_max(miss / np.where(size > 0, size, LD(1))))      # all three exactly 0: no queries in a segment
    print("symmetry %.2e, linearity in g %.2e of the sum of |terms|; asserted 1e-12 each" % (worst_sym, worst_lin))
    assert worst_sym <= 1e-12 and worst_lin <= 1e-12


# ---------------------------------------------------------------- 4. autograd
def _run(v, tt, order):
    return rp.trajectory_eval(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], tt, vel0=v["vel0"], vel2=v["vel2"], order=order)


def test_autograd_order_2():
    fam = tc._families()
    n, k = 257, 33
    for name, sp_big in fam.items():
        sp = _head(sp_big, n)
        tau = tr.query_times(sp, k, 8, exact=False, keep_off_knot=1e-3)
        g_np = hr.gradients(n, k, 9)
        dots, tdot = hr.directions(n, k, 10)
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
        t = _t(tau).requires_grad_()
        leaves = [ins[nm] for nm in NAMES] + [t]
        g = [_t(x).requires_grad_() for x in g_np]
        u = [_t(x) for x in dots] + [_t(tdot)]

        # forward, backward (create_graph False and True) and forward mode: order=1's bits
        first = {}
        for order in (1, 2):
            outs = _run(ins, t, order)
            first[order, "out"] = [o.detach().cpu().numpy() for o in outs]
            for create_graph in (False, True):
                if order == 1 and create_graph:
                    continue
                grads = torch.autograd.grad(outs, leaves, grad_outputs=[x.detach() for x in g], create_graph=create_graph, retain_graph=True)
                first[order, create_graph] = [x.detach().cpu().numpy() for x in grads]
            only = torch.autograd.grad((g[0].detach() * _run(ins, t, order)[0]).sum(), leaves)      # the other two gradients go in as NULL
            first[order, "only"] = [x.cpu().numpy() for x in only]
            with fwAD.dual_level():
                dual = {nm: fwAD.make_dual(ins[nm].detach(), d) for nm, d in zip(NAMES, u[:8])}
                outs = _run(dual, fwAD.make_dual(t.detach(), u[8]), order)
                first[order, "jvp"] = [fwAD.unpack_dual(x).tangent.cpu().numpy() for x in outs]
        for key in ("out", False, "only", "jvp"):
            assert all(_same_bits(a, b) for a, b in zip(first[1, key], first[2, key])), (name, key)
        assert all(_same_bits(a, b) for a, b in zip(first[1, False], first[2, True])), name
        w_bars, w_tau = tc._vjp(sp, tau, g_np)
        assert all(_same_bits(a, b) for a, b in zip(first[2, True], w_bars + [w_tau])), name

        # the double backward of a scalar loss: in the spline inputs and tau the hvp entry, in the first backward's grad_outputs the jvp entry
        grads = torch.autograd.grad(_run(ins, t, 2), leaves, grad_outputs=g, create_graph=True)
        s = sum((gr * x).sum() for gr, x in zip(grads, u))
        second = torch.autograd.grad(s, leaves + g, retain_graph=True)
        want = _all(_hvp(sp, tau, g_np, dots, tdot)) + tc._jvp(sp, tau, dots, tdot)
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(second, want)), name
        # a loss on pos alone, differentiated the second time along pos1 and tau alone: NULL gradients and NULL directions
        grads = torch.autograd.grad(_run(ins, t, 2)[0], [ins["pos1"], t], grad_outputs=g[0].detach(), create_graph=True)
        s = (grads[0] * u[1]).sum() + (grads[1] * u[8]).sum()
        second = torch.autograd.grad(s, leaves)
        want = _all(_hvp(sp, tau, [g_np[0], None, None], [dots[1] if f == 1 else None for f in range(8)], tdot))
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(second, want)), name

        # inputs that do not require grad the second time get None, and a side nothing asks for is not launched
        calls = []
        real_hvp, real_jvp = capi.trajectory_eval_hvp, capi.trajectory_eval_jvp
        capi.trajectory_eval_hvp = lambda *a: (calls.append(("hvp", a[11], a[12])), real_hvp(*a))[1]
        capi.trajectory_eval_jvp = lambda *a: (calls.append(("jvp",)), real_jvp(*a))[1]
        try:
            some = {nm: ins[nm] if nm in ("pos1", "duration0") else ins[nm].detach() for nm in NAMES}
            grads = torch.autograd.grad(_run(some, t.detach(), 2), [some["pos1"], some["duration0"]], grad_outputs=[x.detach() for x in g], create_graph=True)
            torch.autograd.grad((grads[0] * u[1]).sum() + (grads[1] * u[6]).sum(), [some["pos1"], some["duration0"]])
            assert len(calls) == 1 and calls[0][0] == "hvp", calls
            assert [bool(a) for a in calls[0][1]] == [nm in ("pos1", "duration0") for nm in NAMES] and not calls[0][2], calls
            del calls[:]
            grads = torch.autograd.grad(_run({nm: x.detach() for nm, x in ins.items()}, t, 2), [t], grad_outputs=g, create_graph=True)
            got = torch.autograd.grad((grads[0] * u[8]).sum(), g)      # tau alone requires grad on the other side: of the hvp entry, tau's result alone
            assert [c[0] for c in calls] == ["jvp", "hvp"] and not any(calls[1][1]) and calls[1][2], calls
            want = tc._jvp(sp, tau, [None] * 8, tdot)
            assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(got, want)), name
        finally:
            capi.trajectory_eval_hvp, capi.trajectory_eval_jvp = real_hvp, real_jvp

        # against central differences of the device's first-order gradient, one input at a time: step h = 1e-6 max(|x|, 1), the double
        # backward along h against (gradient(x + h) - gradient(x - h)) / 2, normwise per problem over all nine gradients
        def gradient(v, tt):
            with torch.enable_grad():
                v = {nm: x.detach().requires_grad_() for nm, x in v.items()}
                tt = tt.detach().requires_grad_()
                return torch.autograd.grad(_run(v, tt, 1), [v[nm] for nm in NAMES] + [tt], grad_outputs=[x.detach() for x in g])

        grads = torch.autograd.grad(_run(ins, t, 2), leaves, grad_outputs=[x.detach() for x in g], create_graph=True)
        worst = 0.0
        for f in range(9):
            x = leaves[f].detach()
            h = 1e-6 * x.abs().clamp(min=1.0)
            up, dn = dict(ins), dict(ins)
            tu = td = t
            if f < 8:
                up[NAMES[f]], dn[NAMES[f]] = x + h, x - h
            else:
                tu, td = x + h, x - h
            fd = [((a - b) / 2).cpu().numpy() for a, b in zip(gradient(up, tu), gradient(dn, td))]
            got = torch.autograd.grad((grads[f] * h).sum(), leaves, retain_graph=True)
            err = _normwise([a.cpu().numpy() for a in got], fd)
            print("%s: double backward along %s against central differences of the device's gradient, normwise %.2e" % (name, (NAMES + ("tau",))[f], err))
            worst = max(worst, err)
        assert worst <= 1e-6, name

        # second order only
        grads = torch.autograd.grad(_run(ins, t, 2), leaves, grad_outputs=g, create_graph=True)
        (third,) = torch.autograd.grad((grads[5] ** 2).sum(), ins["duration0"], create_graph=True)
        try:
            third.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("a third derivative did not raise")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. end to end
def test_min_time_trajectory_double_backward_against_the_chain_rule():
    """min_time_trajectory(order=2), rest-to-rest: the double backward in the positions of L = S wp pos + wv vel against the chain rule put
    together on the host from the device's own numbers.  With z = (pos, x), x = (vel1, duration0, duration1) the solution, J and Hs its
    Jacobian and second derivatives (min_time_hessian), z_bar the evaluator's gradient (the vjp entry), z_dot = (v, J v) and H z_dot the
    hvp entry along it:  (the Hessian of L) v = [H z_dot]_pos + J^T [H z_dot]_x + S_a z_bar_{x_a} Hs[a] v."""
    n, k = 4096, 8
    p = rp.problems.generate(131, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    pos = [_t(x).requires_grad_() for x in p]
    sol = rp.min_time_hessian(*[x.detach() for x in pos], gap_tol=1e-13)
    vel1, d0, d1 = (x.cpu().numpy() for x in sol[:3])
    status, J, Hs = sol[4].cpu().numpy(), sol[5].cpu().numpy(), sol[6].cpu().numpy()
    usable = np.isfinite(vel1) & np.isfinite(d0) & np.isfinite(d1) & (d0 > 0) & (d1 > 0)
    spl = [None] * 6 + [np.where(usable, d0, 1.0), np.where(usable, d1, 1.0)]
    tau_np = tr.query_times(spl, k, 21, exact=False, keep_off_knot=1e-3)      # fixed times: no part of the solution
    rng = np.random.default_rng(22)
    wp, wv = rng.uniform(0.5, 1.5, (n, k)), rng.uniform(0.5, 1.5, (n, k)) * 0.1
    v = rng.standard_normal((n, 3))
    out = rp.min_time_trajectory(*pos, _t(tau_np), gap_tol=1e-13, order=2)
    vel1, d0, d1 = (x.detach().cpu().numpy() for x in out[3:6])      # the solution the evaluator was given
    loss = (_t(wp) * out[0] + _t(wv) * out[1]).sum()
    grads = torch.autograd.grad(loss, pos, create_graph=True)
    got = torch.autograd.grad(sum((gr * _t(v[:, c])).sum() for c, gr in enumerate(grads)), pos)
    got = np.stack([x.cpu().numpy() for x in got], axis=1)

    zero = np.zeros(n)
    sp = [p[0], p[1], p[2], zero, zero, vel1, d0, d1]
    z_bar, _ = tc._vjp(sp, tau_np, [wp, wv, None], want_tau=False)
    Jv = np.einsum("nab,nb->na", J, v)
    Hz, _ = _hvp(sp, tau_np, [wp, wv, None], [v[:, 0], v[:, 1], v[:, 2], None, None, Jv[:, 0], Jv[:, 1], Jv[:, 2]], None, want_tau=False)
    x_bar, Hz_x = np.stack(z_bar[5:8], axis=1), np.stack(Hz[5:8], axis=1)
    terms = np.concatenate([np.stack(Hz[:3], axis=1)[:, None, :], np.einsum("nab,na->nab", J, Hz_x),
                            np.einsum("na,nabc,nc->nacb", x_bar, Hs, v).reshape(n, 9, 3)], axis=1).astype(LD)      # (n, terms, the three positions)
    want, size = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    fine = usable & ((status & capi.ST_CONVERGED) != 0) & np.isfinite(got).all(axis=1) & np.isfinite(np.asarray(size, dtype=np.float64)).all(axis=1)
    err = np.asarray(np.abs(got - want) / size, dtype=np.float64)[fine]
    print("%d of %d problems converged and finite; double backward against the chain rule: median %.2e, worst %.2e of the sum of |terms|; asserted 1e-12"
          % (int(fine.sum()), n, np.median(err), err.max()))
    assert fine.mean() > 0.95 and err.max() <= 1e-12

    # with end velocities that require grad the solve is first order: the double backward through it raises
    vel0 = _t(zero).requires_grad_()
    few = [x[:64].detach().requires_grad_() for x in pos]
    out = rp.min_time_trajectory(*few, _t(tau_np[:64]), vel0=vel0[:64], gap_tol=1e-13, order=2)
    grads = torch.autograd.grad((out[0] ** 2).sum(), few, create_graph=True)
    try:
        sum(x.sum() for x in grads).backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("a double backward through the solve with end velocities did not raise")
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
